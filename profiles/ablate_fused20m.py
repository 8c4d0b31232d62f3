"""Ablation of k_fused20m: Adam step time of the headline workload with one ingredient compiled out at a time
(-DPINN_ABL=n, see csrc/kernels_fused20m.h; the results of those builds are wrong by construction, only the time is read).

    python profiles/ablate_fused20m.py --build [DIR]     # CPU: one libpinn_hip_abl{n}.so per variant (default DIR: pinn_native/abl, git-ignored)
    python profiles/ablate_fused20m.py [DIR]             # GPU: times them
Since round 5 the -D switches these builds use are not in csrc/ any more.  profiles/ablation_scaffolding.patch holds them; it was
cut from the round-5 sources and is not kept up with csrc/: it reverse-applies to the tree at ee3788e; check that commit out for
the ablation builds (`git checkout ee3788e && git apply -R profiles/ablation_scaffolding.patch`)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pinns-tf2.0_amd")


def build(d):
    """one shared object per variant (hipcc cross-compiles without a GPU; ~2 minutes, eight compiles in parallel);
    the float64 unit is taken from the product build"""
    os.makedirs(d, exist_ok=True)
    hipcc = "/opt/rocm/bin/hipcc"
    common = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-fPIC"]
    procs = [(n, subprocess.Popen(common + ["-DPINN_ABL=%d" % n, "-c", os.path.join(PKG, "csrc", "engine.hip"), "-o",
                                            os.path.join(d, "engine_abl%d.o" % n)],
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)) for n in range(8)]
    for n, p in procs:
        out = p.communicate()[0]
        if p.returncode:
            raise SystemExit("variant %d failed:\n%s" % (n, out[-3000:]))
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", os.path.join(d, "engine_abl%d.o" % n),
                               os.path.join(PKG, "pinn_native", "fused20d_unit.o"), "-o",
                               os.path.join(d, "libpinn_hip_abl%d.so" % n), "-lrccl"])
        os.remove(os.path.join(d, "engine_abl%d.o" % n))


if len(sys.argv) > 1 and sys.argv[1] == "--build":
    build(sys.argv[2] if len(sys.argv) > 2 else os.path.join(PKG, "pinn_native", "abl"))
    raise SystemExit(0)
d = sys.argv[1] if len(sys.argv) > 1 else os.path.join(PKG, "pinn_native", "abl")
NAMES = {0: "product kernel", 1: "no dW matrix instructions", 2: "no group-4 chain / exchange / its barrier",
         3: "workgroup barriers -> LDS waits only", 4: "tanh -> one multiply", 5: "no AGPR stash traffic",
         6: "no adjoint arithmetic in phase A", 7: "no own-group GEMV matrix instructions"}
base = None
for n in range(8):
    lib = os.path.join(d, "libpinn_hip_abl%d.so" % n)
    if not os.path.exists(lib):
        continue
    env = dict(os.environ, PINN_HIP_LIB=lib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "step_time.py"), "f32", "300"], env=env,
                         capture_output=True, text=True).stdout
    us = [float(l.split(":")[2].split("us/step")[0]) for l in out.splitlines() if "us/step" in l]
    if not us:
        print("%d %-44s failed" % (n, NAMES[n])); continue
    t = min(us[1:]) if len(us) > 1 else us[0]
    base = t if n == 0 else base
    print("%d %-44s %6.2f us per Adam step  (%+.2f us)" % (n, NAMES[n], t, t - (base or t)), flush=True)
