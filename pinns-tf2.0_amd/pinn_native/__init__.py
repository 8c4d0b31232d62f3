"""ctypes binding of libpinn_hip.so (C ABI: include/pinn_hip.h) -- the only way the Python
host reaches the GPU.  There is deliberately no CPU fallback: if the HIP library cannot be
loaded or no device is present, construction fails with an explicit error.

    from pinn_native import Engine, build
    eng = Engine(layers, lb, ub, pde="burgers", dtype="f32")
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "csrc")
_REPO = os.path.dirname(os.path.dirname(_HERE))
LIB_PATH = os.environ.get("PINN_HIP_LIB") or os.path.join(_HERE, "libpinn_hip.so")
SOURCES = ["engine.hip", "fused20d_unit.hip", "adr2_20d_unit.hip", "fused20d_api.h", "fused20m_unit.hip", "fused20m_api.h", "kernels_generic.h", "kernels_fused20.h", "kernels_fused20m.h", "kernels_fused20d.h", "kernels_fused20d_kernel.h", "kernels_fused20d_reverse.h", "kernels_wide.h", "kernels_predict20.h",
           "kernels_disc.h", "kernels_sampling.h", "kernels_rad.h", "kernels_tile16.h", "kernels_tile16f.h", "kernels_xgmi.h", "kernels_optim.h", "wave.h", "devbuf.h", "pointsets.h", "optim_host.h"]
HEADER = os.path.join(_REPO, "include", "pinn_hip.h")

PDE_KINDS = {"burgers": 0, "burgers_ide": 1, "schrodinger": 2, "burgers_disc": 3, "burgers_disc_ide": 4, "adr": 5, "adr_ide": 6}
# kinds added after the table above was pinned entry for entry (tests/test_adr_host.py): the discrete-time adr kind
DISC_PDE_KINDS = {"adr_disc": 7, "adr_disc_ide": 8, "adrd_disc": 9}
# ... and the adr equation with b u_t and u_xx + kappa u_tt as one Taylor channel (wave, telegraph, Klein-Gordon, Helmholtz)
ADR2_PDE_KINDS = {"adr2": 10}


def pde_kind(name):
    """name -> enum value of include/pinn_hip.h (PDE_KINDS, DISC_PDE_KINDS, ADR2_PDE_KINDS); ValueError with the tables
    otherwise"""
    for table in (PDE_KINDS, DISC_PDE_KINDS, ADR2_PDE_KINDS):
        if name in table:
            return table[name]
    raise ValueError("pde must be one of %s" % sorted(list(PDE_KINDS) + list(DISC_PDE_KINDS) + list(ADR2_PDE_KINDS)))


DTYPES = {"f32": 0, "f64": 1, "float32": 0, "float64": 1}

ADR_COEFF_NAMES = ("a0", "a1", "nu", "r1", "r2", "r3")     # order of the coefficients, and of the tail of "adr_ide" weights


ADRD_COEFF_NAMES = ADR_COEFF_NAMES + ("d3",)               # "adrd_disc": the dispersion coefficient behind the six
ADR2_COEFF_NAMES = ADR_COEFF_NAMES + ("b", "kappa")        # "adr2": b u_t and -nu (u_xx + kappa u_tt)


def adr_trainable_mask(names_or_mask, names=ADR_COEFF_NAMES):
    """names from ADR_COEFF_NAMES (ADRD_COEFF_NAMES for "adrd_disc": pass it as `names`), or an int mask, passed through
    -> bit mask of pinn_set_pde_trainable"""
    if isinstance(names_or_mask, (int, np.integer)):
        return int(names_or_mask)
    if isinstance(names_or_mask, str):
        names_or_mask = [names_or_mask]
    mask = 0
    for name in names_or_mask:
        if name not in names:
            raise ValueError("unknown adr coefficient %r: choose from %s" % (name, ", ".join(names)))
        mask |= 1 << names.index(name)
    return mask


_c_double_p = ctypes.POINTER(ctypes.c_double)
_c_int_p = ctypes.POINTER(ctypes.c_int)


class PinnNativeError(RuntimeError):
    pass


COMMON_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-fPIC",
                "-mllvm", "-amdgpu-kernarg-preload-count=16"]   # leading argument dwords arrive in SGPRs (no s_load round trip)
UNITS = [("engine.hip", []), ("fused20d_unit.hip", ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]), ("fused20m_unit.hip", []),
         ("adr2_20d_unit.hip", ["-mllvm", "-amdgpu-mfma-vgpr-form=1"])]      # k_adr2_20d: the text of k_fused20d, its flags


def _build_tag():
    """what a library was built from, besides file times: the flags (an ablation / stamps build shares the sources)"""
    return " ".join(COMMON_FLAGS) + " | " + " ; ".join("%s %s" % (u, " ".join(f)) for u, f in UNITS)


def _source_digest():
    """sha256 over the kernel sources and the C header, in SOURCES order: what a library was built from"""
    import hashlib
    h = hashlib.sha256()
    for path in [os.path.join(_CSRC, s) for s in SOURCES] + [HEADER]:
        if os.path.exists(path):
            with open(path, "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()


def library_digest(lib=None):
    """sources-sha256 recorded beside the library when it was built (what the code that RUNS was compiled from); None when
    the flags file is missing"""
    try:
        for line in open((lib or LIB_PATH) + ".flags"):
            if line.startswith("sources-sha256 "):
                return line.split()[1]
    except OSError:
        pass
    return None


def _stale(lib=None):
    """A library is current when the flags file beside it names these flags AND these source contents (a digest, not
    file times: a snapshot copied to another machine keeps no usable time order).  Without a flags file: file times."""
    lib = lib or LIB_PATH
    if not os.path.exists(lib):
        return True
    tag = lib + ".flags"
    if os.path.exists(tag):
        lines = open(tag).read().split("\n")
        digest = [l.split(" ", 1)[1] for l in lines if l.startswith("sources-sha256 ")]
        if lines[0] != _build_tag():
            return True
        if digest:
            return digest[0] != _source_digest()
    built = os.path.getmtime(lib)
    srcs = [os.path.join(_CSRC, s) for s in SOURCES] + [HEADER]
    return any(os.path.exists(s) and os.path.getmtime(s) > built for s in srcs)


def build(force=False, verbose=False, stamps=False):
    """Compile the HIP engine for gfx950 into pinn_native/libpinn_hip.so (in-tree, so the
    shared object travels with the repo snapshot).  hipcc cross-compiles without a GPU.
    stamps=True builds the profiling variant libpinn_hip_stamps.so (-DPINN_STAMPS) instead.
    Safe against concurrent callers (several ranks importing at once): a file lock serialises them, objects go to
    a private temporary directory, the library is moved into place atomically."""
    import fcntl
    import tempfile
    out = LIB_PATH.replace(".so", "_stamps.so") if stamps else LIB_PATH
    if not force and not stamps and not _stale():
        return LIB_PATH
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise PinnNativeError("hipcc not found; cannot build libpinn_hip.so")
    try:
        lock = open(os.path.join(_HERE, ".build.lock"), "w")
    except OSError as e:                          # a read-only install: nothing can be built in place
        raise PinnNativeError("cannot build in %s (%s); build the library where the tree is writable" % (_HERE, e))
    with lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not stamps and not _stale():        # another process built it while we waited
            return LIB_PATH
        # three translation units (compiled concurrently), one shared object: k_fused20d wants its matrix results in
        # VGPRs (csrc/fused20d_api.h), every other kernel keeps hipcc's default allocation; fused20m_unit.hip holds
        # the float32 register-stash kernel at the depths other than 8
        common = [hipcc] + COMMON_FLAGS + (["-DPINN_STAMPS"] if stamps else [])
        digest = _source_digest()
        with tempfile.TemporaryDirectory(prefix="pinn_build_", dir=_HERE) as tmp:
            objs, procs = [], []
            for src, extra in UNITS:
                obj = os.path.join(tmp, os.path.splitext(src)[0] + ".o")
                cmd = common + extra + ["-c", os.path.join(_CSRC, src), "-o", obj]
                if verbose:
                    print(" ".join(cmd))
                procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
                objs.append(obj)
            failures = []
            for cmd, pr in procs:                              # wait for ALL compiles before reporting
                log = pr.communicate()[0]
                if pr.returncode != 0:
                    failures.append("hipcc failed (%s):\n%s" % (" ".join(cmd), log))
            if failures:
                raise PinnNativeError("\n".join(failures))
            tmp_so = os.path.join(tmp, "lib.so")
            cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", tmp_so, "-lrccl"]
            if verbose:
                print(" ".join(cmd))
            res = subprocess.run(cmd, capture_output=True, text=True)
            if res.returncode != 0:
                raise PinnNativeError("hipcc link failed:\n" + res.stdout + res.stderr)
            os.replace(tmp_so, out)
            for obj in objs:                                   # kept for the ablation builds of profiles/ (relinked there)
                os.replace(obj, os.path.join(_HERE, os.path.basename(obj).replace(".o", "_stamps.o" if stamps else ".o")))
        ver = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout.strip().splitlines()
        with open(out + ".flags", "w") as fh:                  # flags + the compiler the kernels were validated with
            fh.write(_build_tag() + ("\n-DPINN_STAMPS" if stamps else "") + "\nsources-sha256 " + digest + "\n" +
                     "\n".join(ver[:3]) + "\n")
    return out


_LIB = None

_SIGNATURES = {
    "pinn_last_error": (ctypes.c_char_p, []),
    "pinn_abi_version": (ctypes.c_int, []),
    "pinn_device_count": (ctypes.c_int, [_c_int_p]),
    "pinn_runtime_versions": (ctypes.c_int, [_c_int_p, _c_int_p, _c_int_p]),
    "pinn_device_info": (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, _c_int_p,
                                        ctypes.POINTER(ctypes.c_int64)]),
    "pinn_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), _c_int_p, ctypes.c_int,
                                   _c_double_p, _c_double_p, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int]),
    "pinn_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "pinn_num_params": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    "pinn_set_collocation": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64,
                                            ctypes.c_int64]),
    "pinn_set_data": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, ctypes.c_int64,
                                     ctypes.c_int64]),
    "pinn_set_boundary": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p,
                                         ctypes.c_int64, ctypes.c_int64]),
    "pinn_set_pde_params": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int]),
    "pinn_get_pde_params": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int]),
    "pinn_set_pde_trainable": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "pinn_set_weights": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64]),
    "pinn_get_weights": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64]),
    "pinn_loss_grad": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, _c_double_p]),
    "pinn_adam_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_double,
                                      ctypes.c_double, ctypes.c_double]),
    "pinn_adam_run_terms": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_double_p]),
    "pinn_adam_run": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_double_p]),
    "pinn_lbfgs_begin": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_double,
                                        ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                        ctypes.c_double]),
    "pinn_lbfgs_run": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_int_p, _c_double_p,
                                      _c_int_p, _c_int_p]),
    "pinn_adam_enqueue": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_int_p]),
    "pinn_adam_enqueue_terms": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_int_p]),
    "pinn_adam_collect": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_double_p]),
    "pinn_lbfgs_enqueue": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_int_p]),
    "pinn_lbfgs_collect": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _c_int_p, _c_double_p,
                                          _c_int_p, _c_int_p]),
    "pinn_weights_snapshot": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "pinn_weights_restore": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "pinn_lbfgs_get_x": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64]),
    "pinn_lbfgs_set_mode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "pinn_predict": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64, _c_double_p]),
    "pinn_error_l2": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, ctypes.c_int64, ctypes.c_int,
                                     _c_double_p]),
    "pinn_get_status": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64),
                                       ctypes.POINTER(ctypes.c_int64)]),
    "pinn_residual": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64]),
    "pinn_residual_at": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64, _c_double_p]),
    "pinn_comm_xgmi_export": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]),
    "pinn_comm_xgmi_attach": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, _c_int_p]),
    "pinn_comm_xgmi_selftest": (ctypes.c_int, [ctypes.c_void_p, _c_int_p]),
    "pinn_comm_benchmark": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _c_double_p]),
    "pinn_comm_set_mode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "pinn_comm_get_mode": (ctypes.c_int, [ctypes.c_void_p, _c_int_p]),
    "pinn_lhs_collocation": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                            ctypes.c_uint64]),
    "pinn_get_collocation": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64]),
    "pinn_rad_collocation": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                            ctypes.c_int64, ctypes.c_uint64, ctypes.c_int, ctypes.c_double]),
    "pinn_disc_set_stage": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_double_p, _c_double_p,
                                           ctypes.c_int64, _c_double_p, ctypes.c_int]),
    "pinn_disc_predict": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_double_p, ctypes.c_int64,
                                         _c_double_p]),
    "pinn_disc_set_periodic": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, ctypes.c_int64, ctypes.c_int]),
    "pinn_comm_unique_id": (ctypes.c_int, [ctypes.c_char_p]),
    "pinn_comm_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int,
                                      ctypes.c_int]),
    "pinn_timing_enable": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "pinn_timing_read": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_int_p]),
    "pinn_sync": (ctypes.c_int, [ctypes.c_void_p]),
    "pinn_set_kernel_path": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "pinn_get_kernel_path": (ctypes.c_int, [ctypes.c_void_p, _c_int_p]),
    "pinn_get_f64_split": (ctypes.c_int, [ctypes.c_void_p, _c_int_p]),
    "pinn_debug_coef_stamps": (ctypes.c_int, [ctypes.POINTER(ctypes.c_longlong)]),
    "pinn_debug_t16f_stamps": (ctypes.c_int, [ctypes.POINTER(ctypes.c_longlong)]),
    "pinn_debug_t16_deal": (ctypes.c_int, [ctypes.c_int, _c_int_p]),
    "pinn_debug_live_buffers": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "pinn_debug_stamps": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong),
                                         ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    # ensembles (include/pinn_hip.h: pinn_ens_*)
    "pinn_ens_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), _c_int_p, ctypes.c_int, _c_double_p,
                                       _c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "pinn_ens_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "pinn_ens_size": (ctypes.c_int, [ctypes.c_void_p, _c_int_p, ctypes.POINTER(ctypes.c_int64)]),
    "pinn_ens_set_collocation": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64, ctypes.c_int64]),
    "pinn_ens_set_data": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, ctypes.c_int64, ctypes.c_int64]),
    "pinn_ens_set_pde_params": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int]),
    "pinn_ens_set_weights": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64]),
    "pinn_ens_get_weights": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64]),
    "pinn_ens_loss_grad": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, _c_double_p]),
    "pinn_ens_adam_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                          ctypes.c_double, _c_double_p]),
    "pinn_ens_adam_run": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_double_p]),
    "pinn_ens_lbfgs_begin": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                            ctypes.c_double, ctypes.c_double, _c_double_p, ctypes.c_int, _c_int_p]),
    "pinn_ens_lbfgs_run": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_int_p, _c_double_p, _c_int_p, _c_int_p]),
    "pinn_ens_predict": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64, _c_double_p]),
    "pinn_ens_error_l2": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, ctypes.c_int64, _c_double_p]),
    "pinn_ens_get_status": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64),
                                           ctypes.POINTER(ctypes.c_int64)]),
    # per-member point sets of an ensemble (include/pinn_hip.h: pinn_ensk_*)
    "pinn_ensk_set_collocation": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64, ctypes.c_int64]),
    "pinn_ensk_set_data": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, ctypes.c_int64, ctypes.c_int64]),
    "pinn_ensk_set_pde_params": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int]),
    "pinn_ensk_lhs_collocation": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                 ctypes.POINTER(ctypes.c_uint64)]),
    # self-adaptive point weights (include/pinn_hip.h: pinn_sa_*)
    "pinn_sa_set_weights": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64, _c_double_p, ctypes.c_int64]),
    "pinn_sa_get_weights": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64, _c_double_p, ctypes.c_int64]),
    "pinn_sa_adam_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double]),
    "pinn_sa_disable": (ctypes.c_int, [ctypes.c_void_p]),
    # per-point loss weights of the adr kind (include/pinn_hip.h: pinn_pw_*)
    "pinn_pw_set": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64, _c_double_p, ctypes.c_int64,
                                   _c_double_p, ctypes.c_int64]),
    "pinn_pw_get": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64, _c_double_p, ctypes.c_int64,
                                   _c_double_p, ctypes.c_int64]),
    "pinn_pw_adam_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double]),
    "pinn_pw_disable": (ctypes.c_int, [ctypes.c_void_p]),
    # Robin points of the adr kind (include/pinn_hip.h: pinn_set_robin, pinn_robin_residual)
    "pinn_set_robin": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p, ctypes.c_int64,
                                      ctypes.c_int64]),
    "pinn_robin_residual": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64]),
    # three-term wall points of the adr2 kind
    "pinn_set_robin3": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p,
                                       ctypes.c_int64, ctypes.c_int64]),
    # source term of the adr kind (include/pinn_hip.h: pinn_set_source)
    "pinn_set_source": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64]),
    # coefficient fields of the adr kind (include/pinn_hip.h: pinn_set_coef_fields)
    "pinn_set_coef_fields": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64]),
    # ensembles of the adr kind (include/pinn_hip.h: pinn_adr_ens_create)
    "pinn_adr_ens_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), _c_int_p, ctypes.c_int, _c_double_p,
                                           _c_double_p, ctypes.c_int, ctypes.c_int]),
    "pinn_adr_ens_set_boundary": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, ctypes.c_int64, ctypes.c_int64]),
    "pinn_adr_ensk_set_boundary": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, ctypes.c_int64, ctypes.c_int64]),
    "pinn_adr_ensk_set_params": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int]),
    "pinn_adr_ens_get_params": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int]),
}


def exported_symbols():
    return sorted(_SIGNATURES)


def _torch_lib_dir():
    """torch/lib of the installed PyTorch-ROCm wheel, found WITHOUT importing torch; None when torch is absent"""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return None
    d = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    return d if os.path.exists(os.path.join(d, "libamdhip64.so")) else None


def _bind_runtime():
    """Decide which HIP runtime + RCCL this process runs on BEFORE the engine is mapped.

    The image holds two sets with the same sonames (libamdhip64.so.7, librccl.so.1, libhsa-runtime64.so.1): /opt/rocm
    (ROCm 7.2, the toolchain the engine is compiled with; the engine's RUNPATH) and the set bundled in torch/lib
    (ROCm 7.0).  The dynamic linker gives the engine whichever is mapped first, and torch maps its own copies by path
    regardless -- an engine that bound /opt/rocm in a process that later imports torch leaves TWO HIP runtimes in one
    process (measured here: heap corruption at exit).  So a process that needs torch.distributed (every rank of a
    data-parallel launch) must bind torch's set, and it must do so before the engine is mapped.
    PINN_HIP_RUNTIME = auto (default): torch's set when this is one rank of WORLD_SIZE > 1 or torch is already
                                       imported, /opt/rocm otherwise (a plain single-process run never needs torch);
                       torch: always torch's set (torch is imported first) -- the same runtime at N = 1 as at N = 8;
                       rocm:  /opt/rocm; refuses to proceed when torch is already in the process.
    runtime_info() reports what was bound; bench.py prints it in every line."""
    import sys
    policy = os.environ.get("PINN_HIP_RUNTIME", "auto").lower()
    if policy not in ("auto", "torch", "rocm"):
        raise PinnNativeError("PINN_HIP_RUNTIME must be auto, torch or rocm (got %r)" % policy)
    have_torch = "torch" in sys.modules
    if policy == "rocm":
        if have_torch:
            raise PinnNativeError("PINN_HIP_RUNTIME=rocm, but torch (with its bundled HIP runtime) is already imported "
                                  "in this process: two HIP runtimes would be mapped")
        return "rocm"
    if policy == "auto" and not have_torch and int(os.environ.get("WORLD_SIZE", "1")) <= 1:
        return "rocm"
    if have_torch:
        return "torch"
    if _torch_lib_dir() is None:
        if policy == "torch":
            raise PinnNativeError("PINN_HIP_RUNTIME=torch, but no PyTorch-ROCm wheel with a bundled runtime is installed")
        return "rocm"
    # import torch itself, not just its libraries: torch's librccl mapped by path BEFORE `import torch` aborts at exit
    # ("double free or corruption", measured in this image even with no engine in the process), and so does the
    # engine-then-torch order under either set.  torch first, engine second is the one order that is clean.
    import torch.distributed  # noqa: F401
    return "torch"


def runtime_info():
    """-> {"hip_runtime", "hip_driver", "rccl_version", "libamdhip64_path", "librccl_path", "libhsa_path", "bound"}: the
    versions the engine's own calls report (pinn_runtime_versions) and the files this process mapped for them"""
    lib = load()
    v = [ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)]
    if lib.pinn_runtime_versions(ctypes.byref(v[0]), ctypes.byref(v[1]), ctypes.byref(v[2])) != 0:
        raise PinnNativeError(lib.pinn_last_error().decode())
    paths = {"libamdhip64": [], "librccl": [], "libhsa-runtime64": []}
    try:
        with open("/proc/self/maps") as fh:
            for line in fh:
                f = line.split()
                if len(f) >= 6 and "x" in f[1]:
                    for key in paths:
                        if os.path.basename(f[5]).startswith(key) and f[5] not in paths[key]:
                            paths[key].append(f[5])
    except OSError:
        pass
    one = lambda k: paths[k][0] if len(paths[k]) == 1 else (paths[k] or None)     # a list = more than one copy mapped (a fault)
    r = v[2].value
    return {"hip_runtime": v[0].value, "hip_driver": v[1].value,
            "rccl_version": "%d.%d.%d" % (r // 10000, (r // 100) % 100, r % 100), "rccl_version_code": r,
            "libamdhip64_path": one("libamdhip64"), "librccl_path": one("librccl"), "libhsa_path": one("libhsa-runtime64"),
            "bound": "torch" if (paths["libamdhip64"] and "/torch/lib/" in paths["libamdhip64"][0]) else "rocm",
            "single_runtime": all(len(paths[k]) <= 1 for k in paths)}


def load():
    """dlopen the engine (building it first if the sources are newer and hipcc exists)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.environ.get("PINN_HIP_LIB") and _stale():     # an explicitly named library (a variant build) is used as it is
        try:
            build()
        except PinnNativeError as e:
            if not os.path.exists(LIB_PATH):
                raise
            import warnings
            warnings.warn("libpinn_hip.so is older than its sources and could not be rebuilt (%s): using the stale "
                          "library" % str(e).splitlines()[0], RuntimeWarning)
    if not os.path.exists(LIB_PATH):
        raise PinnNativeError(
            "libpinn_hip.so is missing (%s): run `python -c 'import __graft_entry__ as g; "
            "g.build()'`.  There is no CPU fallback." % LIB_PATH)
    _bind_runtime()
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def _dp(a):
    return a.ctypes.data_as(_c_double_p)


def _f64(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if shape is not None:
        a = a.reshape(shape)
    return a


def device_count():
    n = ctypes.c_int(0)
    lib = load()
    if lib.pinn_device_count(ctypes.byref(n)) != 0:
        return 0
    return n.value


def live_buffers():
    """(blocks, bytes) of device and pinned host memory the engine owns in this process right now (pinn_debug_live_buffers)"""
    n, b = ctypes.c_int64(0), ctypes.c_int64(0)
    load().pinn_debug_live_buffers(ctypes.byref(n), ctypes.byref(b))
    return n.value, b.value


def device_info(device=0):
    lib = load()
    buf = ctypes.create_string_buffer(256)
    ncu = ctypes.c_int(0)
    mem = ctypes.c_int64(0)
    if lib.pinn_device_info(device, buf, 256, ctypes.byref(ncu), ctypes.byref(mem)) != 0:
        raise PinnNativeError(lib.pinn_last_error().decode())
    return {"name": buf.value.decode(), "compute_units": ncu.value, "hbm_bytes": mem.value}


class Engine(object):
    """One engine context = one GPU, one stream, one network + training set."""

    def __init__(self, layers, lb, ub, pde="burgers", dtype="f32", device=0):
        self._lib = load()
        self._h = ctypes.c_void_p()
        kind = pde_kind(pde)
        if dtype not in DTYPES:
            raise ValueError("dtype must be one of %s" % sorted(DTYPES))
        self.layers = [int(v) for v in layers]
        self.pde, self.dtype = pde, ("f64" if DTYPES[dtype] else "f32")
        self.n_out = self.layers[-1]
        arr = (ctypes.c_int * len(self.layers))(*self.layers)
        self.n_in = self.layers[0]
        lb, ub = _f64(lb, (self.n_in,)), _f64(ub, (self.n_in,))
        self._check(self._lib.pinn_create(ctypes.byref(self._h), arr, len(self.layers), _dp(lb),
                                          _dp(ub), kind, DTYPES[dtype], int(device)))
        n = ctypes.c_int64(0)
        self._check(self._lib.pinn_num_params(self._h, ctypes.byref(n)))
        self.n_params = n.value
        self.n_f = self.n_u = self.n_b = self.n_w = 0
        self._has_source = False
        self._has_coef_fields = False
        self._tickets = {}                # ticket -> its chunk's size (adam_enqueue / lbfgs_enqueue; negative: a terms chunk)
        self._lb_uncollected = 0          # L-BFGS iterations enqueued and not collected yet

    def _check(self, rc):
        if rc != 0:
            raise PinnNativeError("libpinn_hip: %s (code %d)" % (
                self._lib.pinn_last_error().decode(errors="replace"), rc))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.pinn_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- point sets ----------------------------------------------------------------------
    def set_collocation(self, X_f, n_total=None):
        X_f = _f64(X_f).reshape(-1, 2)
        self.n_f = X_f.shape[0]
        self._check(self._lib.pinn_set_collocation(self._h, _dp(X_f), self.n_f,
                                                   self.n_f if n_total is None else int(n_total)))

    def lhs_collocation(self, n_design, seed, first=0, count=None):
        """Draw collocation points [first, first+count) of an n_design-point Latin hypercube on the device."""
        count = int(n_design) - int(first) if count is None else int(count)
        self._check(self._lib.pinn_lhs_collocation(self._h, int(n_design), int(first), count, int(seed)))
        self.n_f = count

    def rad_collocation(self, n_design, seed, n_pool, k=1, c=1.0, first=0, count=None):
        """Draw collocation points [first, first+count) of an n_design-sample set by residual-based adaptive sampling
        (include/pinn_hip.h pinn_rad_collocation): from the n_pool-point LHS design with this seed, with probability
        ~ |f|^k / mean|f|^k + c at the current weights, with replacement."""
        count = int(n_design) - int(first) if count is None else int(count)
        self._check(self._lib.pinn_rad_collocation(self._h, int(n_design), int(first), count, int(n_pool), int(seed),
                                                   int(k), float(c)))
        self.n_f = count

    # ---- self-adaptive point weights (include/pinn_hip.h pinn_sa_*) ------------------------------------------------------
    def sa_set_weights(self, lam_u, lam_f):
        """Enable the weighted loss with one weight per data point (rows of set_data) and per collocation point (rows of
        get_collocation); resets the weights' Adam moments."""
        lam_u, lam_f = _f64(lam_u).ravel(), _f64(lam_f).ravel()
        self._check(self._lib.pinn_sa_set_weights(self._h, _dp(lam_u), lam_u.size, _dp(lam_f), lam_f.size))

    def sa_get_weights(self):
        """-> (lam_u [n_u], lam_f [n_f])"""
        lam_u, lam_f = np.empty(self.n_u, dtype=np.float64), np.empty(self.n_f, dtype=np.float64)
        self._check(self._lib.pinn_sa_get_weights(self._h, _dp(lam_u), lam_u.size, _dp(lam_f), lam_f.size))
        return lam_u, lam_f

    def sa_adam_init(self, lr):
        """ascent rate of the weights in every Adam step (0: held fixed)"""
        self._check(self._lib.pinn_sa_adam_init(self._h, float(lr)))

    def sa_disable(self):
        self._check(self._lib.pinn_sa_disable(self._h))

    # ---- per-point loss weights of the adr kind (include/pinn_hip.h pinn_pw_*) --------------------------------------------
    def pw_set(self, lam_u=None, lam_f=None, lam_b=None):
        """Enable the weighted loss of the adr kind: one weight per data point (rows of set_data), per collocation point
        (rows of get_collocation) and per boundary pair (rows of set_boundary); None = all ones.  Resets the weights' Adam
        moments."""
        arrs = [None if a is None else _f64(a).ravel() for a in (lam_u, lam_f, lam_b)]
        args = []
        for a, n in zip(arrs, (self.n_u, self.n_f, self.n_b)):
            args += [None if a is None else _dp(a), n if a is None else a.size]
        self._check(self._lib.pinn_pw_set(self._h, *args))

    def pw_get(self):
        """-> (lam_u [n_u], lam_f [n_f], lam_b [n_b])"""
        out = [np.empty(n, dtype=np.float64) for n in (self.n_u, self.n_f, self.n_b)]
        self._check(self._lib.pinn_pw_get(self._h, _dp(out[0]), out[0].size, _dp(out[1]), out[1].size,
                                          _dp(out[2]), out[2].size))
        return tuple(out)

    def pw_adam_init(self, rate_u=0.0, rate_f=0.0, rate_b=0.0):
        """ascent rates of the data, collocation and pair weights in every Adam step (0: that class is held fixed)"""
        self._check(self._lib.pinn_pw_adam_init(self._h, float(rate_u), float(rate_f), float(rate_b)))

    def pw_disable(self):
        self._check(self._lib.pinn_pw_disable(self._h))

    def get_collocation(self):
        X = np.empty((self.n_f, 2), dtype=np.float64)
        self._check(self._lib.pinn_get_collocation(self._h, _dp(X), self.n_f))
        return X

    def set_data(self, X_u, u, n_total=None):
        X_u = _f64(X_u).reshape(-1, 2)
        u = _f64(u).reshape(X_u.shape[0], self.n_out)
        self.n_u = X_u.shape[0]
        self._check(self._lib.pinn_set_data(self._h, _dp(X_u), _dp(u), self.n_u,
                                            self.n_u if n_total is None else int(n_total)))

    def set_boundary(self, X_lb, X_ub, n_total=None):
        X_lb, X_ub = _f64(X_lb).reshape(-1, 2), _f64(X_ub).reshape(-1, 2)
        if X_lb.shape != X_ub.shape:
            raise ValueError("X_lb and X_ub must pair up")
        self.n_b = X_lb.shape[0]
        self._check(self._lib.pinn_set_boundary(self._h, _dp(X_lb), _dp(X_ub), self.n_b,
                                                self.n_b if n_total is None else int(n_total)))

    def set_robin(self, X_w, alpha, beta, g, n_total=None):
        """Robin points of the adr kind: alpha u + beta u_x = g at the rows (x, t) of X_w; alpha, beta and g are arrays of one
        value per point or scalars (broadcast).  (1, 0, g) is a Dirichlet value, (0, 1, g) a flux, (h, 1, g) a Robin wall.
        An empty X_w removes the class.  Their part of the loss is added to terms[2] of loss_grad."""
        X_w, cols, n = self._robin_columns(X_w, (("alpha", alpha), ("beta", beta), ("g", g)), n_total)
        if np.any((cols[0] == 0.0) & (cols[1] == 0.0)):
            raise ValueError("a Robin point with alpha = beta = 0 constrains nothing")
        self._check(self._lib.pinn_set_robin(self._h, _dp(X_w), _dp(cols[0]), _dp(cols[1]), _dp(cols[2]), n,
                                             n if n_total is None else int(n_total)))
        self.n_w = n

    @staticmethod
    def _robin_columns(X_w, named, n_total):
        """set_robin's and set_robin3's view of their arguments: X_w as [n, 2], every named column broadcast to [n], all
        finite -> (X_w, columns, n)"""
        X_w = _f64(X_w)
        if X_w.size % 2 or (X_w.ndim > 1 and X_w.shape[-1] != 2):
            raise ValueError("X_w must be [n, 2] rows (x, t), got shape %s" % (X_w.shape,))
        X_w = np.ascontiguousarray(X_w.reshape(-1, 2))
        n = X_w.shape[0]
        cols = []
        for name, v in named:
            v = _f64(v)
            if v.size != 1 and v.size != n:
                raise ValueError("%s must be a scalar or hold one value per Robin point (%d), got %d" % (name, n, v.size))
            v = np.ascontiguousarray(np.broadcast_to(v.reshape(-1), (n,)))
            if not np.all(np.isfinite(v)):
                raise ValueError("%s must be finite" % name)
            cols.append(v)
        if not np.all(np.isfinite(X_w)):
            raise ValueError("X_w must be finite")
        if n_total is not None and int(n_total) < n:
            raise ValueError("n_total (%d) is smaller than the local count (%d)" % (int(n_total), n))
        return X_w, cols, n

    def set_robin3(self, X_w, alpha, beta, gamma, g, n_total=None):
        """Three-term wall points of the adr2 kind: alpha u + beta u_x + gamma u_t = g at the rows (x, t) of X_w, the arguments
        as set_robin's.  (0, 0, 1, v0) is an initial velocity (or a Neumann wall y = const of a 2-D problem), (0, c, 1, 0)
        the absorbing wall u_t + c u_x = 0.  An empty X_w removes the class."""
        X_w, cols, n = self._robin_columns(X_w, (("alpha", alpha), ("beta", beta), ("gamma", gamma), ("g", g)), n_total)
        if np.any((cols[0] == 0.0) & (cols[1] == 0.0) & (cols[2] == 0.0)):
            raise ValueError("a wall point with alpha = beta = gamma = 0 constrains nothing")
        self._check(self._lib.pinn_set_robin3(self._h, _dp(X_w), _dp(cols[0]), _dp(cols[1]), _dp(cols[2]), _dp(cols[3]), n,
                                              n if n_total is None else int(n_total)))
        self.n_w = n

    def set_source(self, s):
        """Source term of the adr kind: f_i = N[u](x_i, t_i) - s[i] at collocation point i (the rows of get_collocation).
        None removes it.  A redraw of the collocation set makes a present source stale: evaluations are refused until
        set_source is called again with values at the new points (get_collocation still works then)."""
        if s is None:
            self._check(self._lib.pinn_set_source(self._h, None, 0))
            self._has_source = False
            return
        s = np.ascontiguousarray(_f64(s).reshape(-1))
        if s.size != self.n_f:
            raise ValueError("the source term must hold one value per collocation point (%d), got %d" % (self.n_f, s.size))
        if s.size == 0:
            raise ValueError("the source term is empty (None removes a source)")
        if not np.all(np.isfinite(s)):
            raise ValueError("the source term must be finite")
        self._check(self._lib.pinn_set_source(self._h, _dp(s), s.size))
        self._has_source = True

    @property
    def has_source(self):
        """a source term is present (set_source), stale or not"""
        return bool(getattr(self, "_has_source", False))

    def set_coef_fields(self, K):
        """Coefficient fields of the adr kind: row i of K [n_f, 6] holds (a0, a1, nu, r1, r2, r3) of collocation point i (the
        rows of get_collocation); the constants of set_pde_params are not read while fields are present.  None removes
        them.  A redraw of the collocation set makes present fields stale: evaluations are refused until set_coef_fields is
        called again with rows at the new points (get_collocation still works then)."""
        if K is None:
            self._check(self._lib.pinn_set_coef_fields(self._h, None, 0))
            self._has_coef_fields = False
            return
        K = _f64(K)
        if K.ndim != 2 or K.shape[1] != 6:
            raise ValueError("the coefficient fields must be an [n_f, 6] array (a0, a1, nu, r1, r2, r3 per collocation point), "
                             "got shape %s" % (K.shape,))
        K = np.ascontiguousarray(K)
        if K.shape[0] != self.n_f:
            raise ValueError("the coefficient fields must hold one row per collocation point (%d), got %d" % (self.n_f, K.shape[0]))
        if K.shape[0] == 0:
            raise ValueError("the coefficient fields are empty (None removes them)")
        if not np.all(np.isfinite(K)):
            raise ValueError("the coefficient fields must be finite")
        self._check(self._lib.pinn_set_coef_fields(self._h, _dp(K), K.shape[0]))
        self._has_coef_fields = True

    @property
    def has_coef_fields(self):
        """coefficient fields are present (set_coef_fields), stale or not"""
        return bool(getattr(self, "_has_coef_fields", False))

    def robin_residual(self):
        """r_j = alpha_j u + beta_j u_x - g_j at the Robin points, current weights -> [n_w]"""
        r = np.empty(self.n_w, dtype=np.float64)
        self._check(self._lib.pinn_robin_residual(self._h, _dp(r), r.size))
        return r

    def set_pde_params(self, *p):
        p = _f64(p)
        self._check(self._lib.pinn_set_pde_params(self._h, _dp(p), p.size))

    def get_pde_params(self):
        """the current raw equation parameters: six coefficients (a0, a1, nu, r1, r2, r3) for "adr", "adr_disc", "adr_ide"
        and "adr_disc_ide" (the last two: the trained values, nu = exp of the stored log nu), seven (.., d3) for "adrd_disc"
        (nu = 0 where it was set to 0), eight (.., b, kappa) for "adr2", [nu] otherwise"""
        p = np.empty(8 if self.pde == "adr2" else 7 if self.pde == "adrd_disc" else 6 if self.pde in ("adr", "adr_ide", "adr_disc", "adr_disc_ide") else 1,
                     dtype=np.float64)
        self._check(self._lib.pinn_get_pde_params(self._h, _dp(p), p.size))
        return p

    def set_pde_trainable(self, names_or_mask):
        """pde "adr_ide" and "adr_disc_ide": which coefficients are trained -- names from ADR_COEFF_NAMES or a bit mask (bit k = name k); the
        others stay frozen at their values, bit for bit.  pde "adrd_disc": names from ADRD_COEFF_NAMES (bit 6 = d3)"""
        names = ADRD_COEFF_NAMES if self.pde == "adrd_disc" else ADR_COEFF_NAMES
        self._check(self._lib.pinn_set_pde_trainable(self._h, adr_trainable_mask(names_or_mask, names)))

    # ---- weights ---------------------------------------------------------------------------
    def set_weights(self, w):
        w = _f64(w).ravel()
        self._check(self._lib.pinn_set_weights(self._h, _dp(w), w.size))

    def get_weights(self):
        w = np.empty(self.n_params, dtype=np.float64)
        self._check(self._lib.pinn_get_weights(self._h, _dp(w), w.size))
        return w

    # ---- evaluation ------------------------------------------------------------------------
    def loss_grad(self, want_grad=True):
        loss = ctypes.c_double(0.0)
        terms = np.zeros(3, dtype=np.float64)
        grad = np.empty(self.n_params, dtype=np.float64) if want_grad else None
        self._check(self._lib.pinn_loss_grad(self._h, ctypes.byref(loss),
                                             _dp(grad) if want_grad else None, _dp(terms)))
        return loss.value, grad, terms

    # ---- discrete-time models (pde "burgers_disc", "burgers_disc_ide", "adr_disc", "adr_disc_ide", "adrd_disc") -------------
    def disc_set_stage(self, stage, x, target, M=None):
        """Stage set `stage` (0/1): points x [n], targets [n] (broadcast over the outputs), M [n_out, q] =
        step-scaled IRK table or None (no IRK term).  See include/pinn_hip.h."""
        x, target = _f64(x).ravel(), _f64(target).ravel()
        if x.size != target.size:
            raise ValueError("x and target must pair up")
        q = 0
        if M is not None:
            M = _f64(M)
            if M.ndim != 2 or M.shape[0] != self.n_out:
                raise ValueError("M must be [n_out, q]")
            q = M.shape[1]
        self._check(self._lib.pinn_disc_set_stage(self._h, int(stage), _dp(x), _dp(target), x.size,
                                                  _dp(M) if M is not None else None, q))

    def disc_set_periodic(self, x_lb, x_ub, order=1):
        """Periodic pairs of pde "adr_disc", "adr_disc_ide" and "adrd_disc": x_lb[i] with x_ub[i]; every output's value (order 0) or value and slope
        (order 1) difference, squared and summed, is added to the loss and reported in terms[2].  Empty arrays remove the
        pairs.  See include/pinn_hip.h."""
        x_lb, x_ub = _f64(x_lb).ravel(), _f64(x_ub).ravel()
        if x_lb.size != x_ub.size:
            raise ValueError("x_lb and x_ub must pair up")
        self._check(self._lib.pinn_disc_set_periodic(self._h, _dp(x_lb), _dp(x_ub), x_lb.size, int(order)))

    def disc_predict(self, stage, x):
        x = _f64(x).ravel()
        out = np.empty((x.size, self.n_out), dtype=np.float64)
        self._check(self._lib.pinn_disc_predict(self._h, int(stage), _dp(x), x.size, _dp(out)))
        return out

    def predict(self, X):
        X = _f64(X).reshape(-1, self.n_in)
        out = np.empty((X.shape[0], self.n_out), dtype=np.float64)
        self._check(self._lib.pinn_predict(self._h, _dp(X), X.shape[0], _dp(out)))
        return out

    def error_l2(self, X, ref, modulus=False):
        """||ref - model(X)||_2 / ||ref||_2 reduced on the device (the scripts' error metric).  modulus=True compares
        |h| = sqrt(sum_o out_o^2) with ref [n] (Schrodinger)."""
        X = _f64(X).reshape(-1, self.n_in)
        ref = _f64(ref).reshape(-1) if modulus else _f64(ref).reshape(X.shape[0], self.n_out)
        if ref.shape[0] != X.shape[0]:
            raise ValueError("ref must hold one row per point")
        err = ctypes.c_double(0.0)
        self._check(self._lib.pinn_error_l2(self._h, _dp(X), _dp(ref), X.shape[0], 1 if modulus else 0,
                                            ctypes.byref(err)))
        return err.value

    def status(self):
        """(loss+grad evaluations so far, 1-based number of the first one with a non-finite loss or 0)"""
        n, bad = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._lib.pinn_get_status(self._h, ctypes.byref(n), ctypes.byref(bad)))
        return n.value, bad.value

    def residual(self):
        n = self.n_u if self.pde == "burgers_ide" else self.n_f
        f = np.empty((n, self.n_out), dtype=np.float64)
        self._check(self._lib.pinn_residual(self._h, _dp(f), n))
        return f

    def residual_at(self, X, source=None):
        """f_model at arbitrary points X [n, 2] -> [n, n_out].  A context with a source term (set_source) cannot know s at
        foreign points: pass source = s(X) [n], subtracted here from the operator part the library returns."""
        X = _f64(X).reshape(-1, 2)
        if source is None and self.has_source:
            raise ValueError("residual_at: this context holds a source term; pass source = s at the rows of X")
        if source is not None:
            source = _f64(source).reshape(-1)
            if source.size != X.shape[0]:
                raise ValueError("residual_at: source must hold one value per point (%d), got %d" % (X.shape[0], source.size))
        f = np.empty((X.shape[0], self.n_out), dtype=np.float64)
        self._check(self._lib.pinn_residual_at(self._h, _dp(X), X.shape[0], _dp(f)))
        return f if source is None else f - source.reshape(-1, 1)

    # ---- optimisers ------------------------------------------------------------------------
    def adam_init(self, lr, beta1=0.9, beta2=0.999, eps=1e-7):
        self._check(self._lib.pinn_adam_init(self._h, lr, beta1, beta2, eps))

    def adam_run_terms(self, n_steps):
        """[n_steps, 3] = (residual, data, boundary) loss parts before each update."""
        terms = np.empty((max(int(n_steps), 1), 3), dtype=np.float64)
        self._check(self._lib.pinn_adam_run_terms(self._h, int(n_steps), _dp(terms)))
        return terms[:n_steps]

    def adam_run(self, n_steps, want_losses=True):
        if not want_losses:
            self._check(self._lib.pinn_adam_run(self._h, int(n_steps), None))
            return None
        losses = np.empty(max(int(n_steps), 1), dtype=np.float64)
        self._check(self._lib.pinn_adam_run(self._h, int(n_steps), _dp(losses)))
        return losses[:n_steps]

    # -- the same loops with the host one chunk behind the GPU (include/pinn_hip.h: pinn_*_enqueue / _collect) --------
    MAX_IN_FLIGHT = 4

    def adam_enqueue(self, n_steps, terms=False):
        """n_steps Adam iterations into the stream -> ticket (returns at once); adam_collect(ticket) -> their losses
        ([n] sums, or with terms=True the [n, 3] parts (residual, data, boundary) of adam_run_terms)"""
        t = ctypes.c_int(0)
        fn = self._lib.pinn_adam_enqueue_terms if terms else self._lib.pinn_adam_enqueue
        self._check(fn(self._h, int(n_steps), ctypes.byref(t)))
        self._tickets[t.value] = -int(n_steps) if terms else int(n_steps)      # (negative: a terms chunk)
        return t.value

    def adam_collect(self, ticket):
        n = self._tickets[ticket]
        terms, n = n < 0, abs(n)
        losses = np.empty((max(n, 1), 3) if terms else max(n, 1), dtype=np.float64)
        self._check(self._lib.pinn_adam_collect(self._h, int(ticket), _dp(losses)))
        del self._tickets[ticket]
        return losses[:n]

    def lbfgs_enqueue(self, n_iters):
        t = ctypes.c_int(0)
        self._check(self._lib.pinn_lbfgs_enqueue(self._h, int(n_iters), ctypes.byref(t)))
        self._lb_uncollected += int(n_iters)
        self._tickets[t.value] = int(n_iters)
        return t.value

    def lbfgs_collect(self, ticket):
        """-> (iters, losses, done) of the log entries that became due with this chunk"""
        cap = self._lb_uncollected + 1            # every iteration enqueued since the last collect may have logged one entry
        iters = np.zeros(cap, dtype=np.int32)
        losses = np.zeros(cap, dtype=np.float64)
        n_logged, done = ctypes.c_int(0), ctypes.c_int(0)
        self._check(self._lib.pinn_lbfgs_collect(self._h, int(ticket), cap, iters.ctypes.data_as(_c_int_p), _dp(losses),
                                                 ctypes.byref(n_logged), ctypes.byref(done)))
        del self._tickets[ticket]
        self._lb_uncollected = sum(abs(v) for v in self._tickets.values())
        k = n_logged.value
        return iters[:k].copy(), losses[:k].copy(), done.value

    N_SNAPSHOTS = 4

    def weights_snapshot(self, slot):
        """device-side copy of the weights into slot 0..3, in stream order (no synchronisation)"""
        self._check(self._lib.pinn_weights_snapshot(self._h, int(slot)))

    def weights_restore(self, slot):
        self._check(self._lib.pinn_weights_restore(self._h, int(slot)))

    def lbfgs_begin(self, max_iter, lr, n_corr, tol_fun, tol_x=1e-19, max_eval=0.0):
        self._tickets, self._lb_uncollected = {}, 0          # chunks still in flight are dropped by the engine (a restart)
        self._lb_max_iter = int(max_iter)
        self._check(self._lib.pinn_lbfgs_begin(self._h, int(max_iter), lr, int(n_corr), tol_fun,
                                               tol_x, max_eval))

    def lbfgs_set_mode(self, mode):
        self._check(self._lib.pinn_lbfgs_set_mode(self._h, int(mode)))

    def lbfgs_run(self, n_iters):
        cap = max(int(n_iters), 1)                # n_iters entries: the tight bound of the synchronous call (include/pinn_hip.h)
        iters = np.zeros(cap, dtype=np.int32)
        losses = np.zeros(cap, dtype=np.float64)
        n_logged, done = ctypes.c_int(0), ctypes.c_int(0)
        self._check(self._lib.pinn_lbfgs_run(self._h, int(n_iters),
                                             iters.ctypes.data_as(_c_int_p), _dp(losses),
                                             ctypes.byref(n_logged), ctypes.byref(done)))
        k = n_logged.value
        return iters[:k].copy(), losses[:k].copy(), done.value

    def lbfgs_x(self):
        x = np.empty(self.n_params, dtype=np.float64)
        self._check(self._lib.pinn_lbfgs_get_x(self._h, _dp(x), x.size))
        return x

    # ---- multi-GPU -------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        lib = load()
        buf = ctypes.create_string_buffer(128)
        if lib.pinn_comm_unique_id(buf) != 0:
            raise PinnNativeError(lib.pinn_last_error().decode())
        return buf.raw

    def comm_init(self, unique_id, n_ranks, rank):
        self._check(self._lib.pinn_comm_init(self._h, bytes(unique_id), int(n_ranks), int(rank)))

    # ---- measurement -----------------------------------------------------------------------
    def comm_xgmi_export(self, n_ranks, rank):
        buf = ctypes.create_string_buffer(64)
        self._check(self._lib.pinn_comm_xgmi_export(self._h, int(n_ranks), int(rank), buf))
        return buf.raw

    def comm_xgmi_attach(self, handles):
        """handles: list of the 64-byte handles of all ranks, rank order.  True if every peer mailbox got mapped."""
        blob = b"".join(handles)
        ok = ctypes.c_int(0)
        self._check(self._lib.pinn_comm_xgmi_attach(self._h, blob, len(handles), ctypes.byref(ok)))
        return bool(ok.value)

    def comm_xgmi_selftest(self):
        ok = ctypes.c_int(0)
        self._check(self._lib.pinn_comm_xgmi_selftest(self._h, ctypes.byref(ok)))
        return bool(ok.value)

    def comm_benchmark(self, mode, iters=200):
        us = ctypes.c_double(0.0)
        self._check(self._lib.pinn_comm_benchmark(self._h, {"rccl": 1, "mailbox": 2}.get(mode, mode), int(iters),
                                                  ctypes.byref(us)))
        return us.value

    def comm_set_mode(self, mode):
        self._check(self._lib.pinn_comm_set_mode(self._h, {"rccl": 1, "mailbox": 2}.get(mode, mode)))

    def comm_mode(self):
        m = ctypes.c_int(0)
        self._check(self._lib.pinn_comm_get_mode(self._h, ctypes.byref(m)))
        return {0: "none", 1: "rccl", 2: "mailbox"}[m.value]

    def timing_enable(self, max_evals, every=1):
        self._check(self._lib.pinn_timing_enable(self._h, int(max_evals), int(every)))

    def timing_read(self):
        ms = np.zeros(5, dtype=np.float64)
        n = ctypes.c_int(0)
        self._check(self._lib.pinn_timing_read(self._h, _dp(ms), ctypes.byref(n)))
        return {"fwd_ms": ms[0], "sweeps_ms": ms[1], "eval_ms": ms[2], "empty_bracket_ms": ms[3],
                "kernel_exact": bool(ms[4]), "n": n.value}

    def sync(self):
        self._check(self._lib.pinn_sync(self._h))

    def set_kernel_path(self, path):
        self._check(self._lib.pinn_set_kernel_path(self._h, int(path)))

    def debug_stamps(self):
        """(profiling build) -> int64 array [n_waves, 32] of s_memtime ticks for one evaluation"""
        n_wg = (2 * self.n_b + self.n_u + self.n_f + getattr(self, "n_w", 0) + 63) // 64
        n_wg += (n_wg + 1) // 2                # a split launch of path 7 (f64_split): the helper workgroups' stamps follow
        buf = np.zeros((n_wg * 4, 32), dtype=np.int64)
        n = ctypes.c_int64(0)
        self._check(self._lib.pinn_debug_stamps(
            self._h, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), buf.size, ctypes.byref(n)))
        return buf[:n.value]

    def kernel_path(self):
        p = ctypes.c_int(0)
        self._check(self._lib.pinn_get_kernel_path(self._h, ctypes.byref(p)))
        return p.value

    @property
    def f64_split(self):
        """True when the next evaluation takes the split one-tile launch of kernel path 7 (include/pinn_hip.h:
        pinn_get_f64_split; environment PINN_F64_SPLIT = auto / 0 / 1, read when the engine is created).  Read-only."""
        p = ctypes.c_int(0)
        self._check(self._lib.pinn_get_f64_split(self._h, ctypes.byref(p)))
        return bool(p.value)


class Ensemble(object):
    """K members of one float64 Burgers net (kernel path 7) trained side by side (include/pinn_hip.h: pinn_ens_*), on one
    shared point set or, once a per-member set, viscosity or hypercube is given, on one set per member (pinn_ensk_*).
    Everything per member carries a leading K axis; member k ends bit-identical to an Engine trained alone from the same
    weights, points and viscosity with the same calls."""

    MAX_MEMBERS = 64

    def __init__(self, layers, lb, ub, n_members, pde="burgers", dtype="f64", device=0):
        self._lib = load()
        self._h = ctypes.c_void_p()
        kind = pde_kind(pde)
        if dtype not in DTYPES:
            raise ValueError("dtype must be one of %s" % sorted(DTYPES))
        self.layers = [int(v) for v in layers]
        self.pde = pde
        arr = (ctypes.c_int * len(self.layers))(*self.layers)
        lb, ub = _f64(lb, (2,)), _f64(ub, (2,))
        self._check(self._create(arr, lb, ub, kind, DTYPES[dtype], int(device), int(n_members)))
        k, n = ctypes.c_int(0), ctypes.c_int64(0)
        self._check(self._lib.pinn_ens_size(self._h, ctypes.byref(k), ctypes.byref(n)))
        self.n_members, self.n_params = k.value, n.value

    def _create(self, arr, lb, ub, kind, dtype, device, n_members):
        return self._lib.pinn_ens_create(ctypes.byref(self._h), arr, len(self.layers), _dp(lb), _dp(ub), kind, dtype,
                                         device, n_members)

    def _check(self, rc):
        if rc != 0:
            raise PinnNativeError("libpinn_hip: %s (code %d)" % (
                self._lib.pinn_last_error().decode(errors="replace"), rc))

    f64_split = False      # an ensemble launch never takes the split one-tile plan of a solo Engine (Engine.f64_split)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.pinn_ens_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- point sets and PDE parameters: shared, or one per member ----------------------------------
    def _per_member(self, a, what, cols):
        """a [n, cols] (shared) -> (a, False); a [K, n, cols] (one per member) -> (a, True); anything else: ValueError"""
        a = _f64(a)
        if a.ndim == 3:
            if a.shape[0] != self.n_members or a.shape[2] != cols:
                raise ValueError("%s: per-member array must be [K=%d, n, %d], got %s" % (what, self.n_members, cols,
                                                                                       a.shape))
            return a, True
        if a.size % cols:
            raise ValueError("%s: array must be [n, %d] (shared) or [K=%d, n, %d] (per member), got %s" % (
                what, cols, self.n_members, cols, a.shape))
        return a.reshape(-1, cols), False

    def set_collocation(self, X_f, n_total=None):
        """X_f [n, 2] for every member, or [K, n, 2]: member k's own set"""
        X_f, per = self._per_member(X_f, "X_f", 2)
        n = X_f.shape[-2]
        nt = n if n_total is None else int(n_total)
        fn = self._lib.pinn_ensk_set_collocation if per else self._lib.pinn_ens_set_collocation
        self._check(fn(self._h, _dp(X_f), n, nt))

    def set_data(self, X_u, u, n_total=None):
        """X_u [n, 2], u [n, 1] for every member, or [K, n, 2], [K, n, 1]: member k's own data"""
        X_u, per = self._per_member(X_u, "X_u", 2)
        n = X_u.shape[-2]
        u = _f64(u)
        want = (self.n_members, n, 1) if per else (n, 1)
        if u.size != n * (self.n_members if per else 1) or (per and u.shape[:2] != want[:2]):
            raise ValueError("u: expected %s to go with X_u %s, got %s" % (want, X_u.shape, u.shape))
        u = u.reshape(want)
        nt = n if n_total is None else int(n_total)
        fn = self._lib.pinn_ensk_set_data if per else self._lib.pinn_ens_set_data
        self._check(fn(self._h, _dp(X_u), _dp(u), n, nt))

    def set_pde_params(self, *p):
        """nu for every member, or nu [K]: member k's own (identification: accepted and unused)"""
        if len(p) == 1 and np.ndim(p[0]) == 1:
            nu = _f64(p[0])
            if nu.shape != (self.n_members,):
                raise ValueError("nu: per-member array must be [K=%d], got %s" % (self.n_members, nu.shape))
            self._check(self._lib.pinn_ensk_set_pde_params(self._h, _dp(nu), nu.size))
            return
        p = _f64(p)
        self._check(self._lib.pinn_ens_set_pde_params(self._h, _dp(p), p.size))

    def lhs_collocation(self, n_design, seeds, first=0, count=None):
        """Engine.lhs_collocation for every member in one launch: member k draws points [first, first+count) of the
        n_design-point Latin hypercube with seed seeds[k]"""
        seeds = np.asarray(seeds)
        if seeds.shape != (self.n_members,) or not np.issubdtype(seeds.dtype, np.integer):
            raise ValueError("seeds: expected [K=%d] integers, got %s %s" % (self.n_members, seeds.shape, seeds.dtype))
        seeds = np.ascontiguousarray(seeds.astype(np.uint64))
        count = int(n_design) - int(first) if count is None else int(count)
        self._check(self._lib.pinn_ensk_lhs_collocation(self._h, int(n_design), int(first), count,
                                                        seeds.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))

    # ---- per-member weights --------------------------------------------------------------------
    def set_weights(self, W):
        W = _f64(W).reshape(self.n_members, self.n_params)
        self._check(self._lib.pinn_ens_set_weights(self._h, _dp(W), W.size))

    def get_weights(self):
        W = np.empty((self.n_members, self.n_params), dtype=np.float64)
        self._check(self._lib.pinn_ens_get_weights(self._h, _dp(W), W.size))
        return W

    def loss_grad(self, want_grad=True):
        """-> losses [K], grads [K, P] (or None), terms [K, 3]"""
        losses = np.empty(self.n_members, dtype=np.float64)
        terms = np.empty((self.n_members, 3), dtype=np.float64)
        grads = np.empty((self.n_members, self.n_params), dtype=np.float64) if want_grad else None
        self._check(self._lib.pinn_ens_loss_grad(self._h, _dp(losses), _dp(grads) if want_grad else None, _dp(terms)))
        return losses, grads, terms

    # ---- optimisers ------------------------------------------------------------------------------
    def adam_init(self, lr, beta1=0.9, beta2=0.999, eps=1e-7):
        """lr: a number, or one per member"""
        lr_k = np.broadcast_to(_f64(lr), (self.n_members,)).copy()
        self._check(self._lib.pinn_ens_adam_init(self._h, float(lr_k[0]), beta1, beta2, eps, _dp(lr_k)))

    def adam_run(self, n_steps):
        """-> losses [n_steps, K], each member's loss before update i"""
        losses = np.empty((max(int(n_steps), 1), self.n_members), dtype=np.float64)
        self._check(self._lib.pinn_ens_adam_run(self._h, int(n_steps), _dp(losses)))
        return losses[:n_steps]

    def lbfgs_begin(self, max_iter, lr, n_corr, tol_fun, tol_x=1e-19, max_eval=0.0):
        """max_iter, lr: a number, or one per member; n_corr, tol_fun, tol_x, max_eval are shared"""
        it_k = np.ascontiguousarray(np.broadcast_to(np.asarray(max_iter, dtype=np.int32), (self.n_members,)))
        lr_k = np.broadcast_to(_f64(lr), (self.n_members,)).copy()
        self._check(self._lib.pinn_ens_lbfgs_begin(self._h, int(n_corr), tol_fun, tol_x, max_eval, float(lr_k[0]),
                                                   _dp(lr_k), int(it_k[0]), it_k.ctypes.data_as(_c_int_p)))

    def lbfgs_run(self, n_iters):
        """-> (iters, losses, done): lists of K arrays of the log entries each member produced, done [K]"""
        K, cap = self.n_members, int(n_iters) + 1     # the rows' length in the C API; at most n_iters entries come back, as solo
        iters = np.zeros((K, cap), dtype=np.int32)
        losses = np.zeros((K, cap), dtype=np.float64)
        n_logged, done = np.zeros(K, dtype=np.int32), np.zeros(K, dtype=np.int32)
        self._check(self._lib.pinn_ens_lbfgs_run(self._h, int(n_iters), iters.ctypes.data_as(_c_int_p), _dp(losses),
                                                 n_logged.ctypes.data_as(_c_int_p), done.ctypes.data_as(_c_int_p)))
        return ([iters[k, :n_logged[k]].copy() for k in range(K)], [losses[k, :n_logged[k]].copy() for k in range(K)],
                done)

    # ---- evaluation ------------------------------------------------------------------------------
    def predict(self, X):
        """-> [K, n, 1]"""
        X = _f64(X).reshape(-1, 2)
        out = np.empty((self.n_members, X.shape[0], 1), dtype=np.float64)
        self._check(self._lib.pinn_ens_predict(self._h, _dp(X), X.shape[0], _dp(out)))
        return out

    def error_l2(self, X, ref):
        """-> [K] relative L2 errors of each member's prediction at X against ref"""
        X = _f64(X).reshape(-1, 2)
        ref = _f64(ref).reshape(X.shape[0], 1)
        err = np.empty(self.n_members, dtype=np.float64)
        self._check(self._lib.pinn_ens_error_l2(self._h, _dp(X), _dp(ref), X.shape[0], _dp(err)))
        return err

    def status(self):
        """-> (evaluations [K], first non-finite evaluation [K], 0 = none)"""
        n = np.zeros(self.n_members, dtype=np.int64)
        bad = np.zeros(self.n_members, dtype=np.int64)
        self._check(self._lib.pinn_ens_get_status(self._h, n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                  bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return n, bad


class AdrEnsemble(Ensemble):
    """K members of one float64 net of the adr kind (kernel path 7) trained side by side (include/pinn_hip.h:
    pinn_adr_ens_create): Ensemble's surface, and every member with its own six coefficients (a0, a1, nu, r1, r2, r3) and,
    per member or shared, periodic boundary pairs.  Member k ends bit-identical to an Engine(pde="adr") trained alone from
    the same weights, coefficients and points with the same calls."""

    def __init__(self, layers, lb, ub, n_members, device=0):
        Ensemble.__init__(self, layers, lb, ub, n_members, pde="adr", dtype="f64", device=device)

    def _create(self, arr, lb, ub, kind, dtype, device, n_members):
        return self._lib.pinn_adr_ens_create(ctypes.byref(self._h), arr, len(self.layers), _dp(lb), _dp(ub), device,
                                             n_members)

    def set_boundary(self, X_lb, X_ub, n_total=None):
        """periodic pairs: X_lb, X_ub [n, 2] for every member, or [K, n, 2]: member k's own pairs"""
        X_lb, per = self._per_member(X_lb, "X_lb", 2)
        X_ub, per_ub = self._per_member(X_ub, "X_ub", 2)
        if per != per_ub or X_lb.shape != X_ub.shape:
            raise ValueError("X_lb %s and X_ub %s must have one shape" % (X_lb.shape, X_ub.shape))
        n = X_lb.shape[-2]
        nt = n if n_total is None else int(n_total)
        fn = self._lib.pinn_adr_ensk_set_boundary if per else self._lib.pinn_adr_ens_set_boundary
        self._check(fn(self._h, _dp(X_lb), _dp(X_ub), n, nt))

    def set_pde_params(self, *p):
        """six numbers (a0, a1, nu, r1, r2, r3) for every member, or [K, 6]: member k's own row"""
        if len(p) == 1 and np.ndim(p[0]) == 2:
            rows = _f64(p[0])
            if rows.shape != (self.n_members, 6):
                raise ValueError("coefficients: per-member array must be [K=%d, 6], got %s" % (self.n_members, rows.shape))
            self._check(self._lib.pinn_adr_ensk_set_params(self._h, _dp(rows), self.n_members))
            return
        p = _f64(p).reshape(-1)
        self._check(self._lib.pinn_ens_set_pde_params(self._h, _dp(p), p.size))

    def get_pde_params(self):
        """-> [K, 6]"""
        rows = np.empty((self.n_members, 6), dtype=np.float64)
        self._check(self._lib.pinn_adr_ens_get_params(self._h, _dp(rows), self.n_members))
        return rows
