"""Bit identity of two builds of the library on short trainings that bench.py does not cover: identification on kernel path 7
(depth 8) and Burgers inference at depths 4 and 6, float64, one tile per workgroup.

    [PINN_HIP_LIB=<variant .so>] python profiles/onetile_fold_bits.py dump DIR
        -> DIR/<workload>/{weights,adam_losses,lbfgs_losses,loss,loss_terms,grad}.npy after 40 Adam + 60 L-BFGS steps
    python profiles/onetile_fold_bits.py compare DIR_A DIR_B
        -> every .npy below both directories (bench.py --dump-outputs DIR/bench included) compared with np.array_equal;
           exit status 1 on any difference

Results: profiles/onetile_fold_bits.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pinns-tf2.0_amd"), os.path.join(ROOT, "tests", "helpers")):
    sys.path.insert(0, p)


def dump(out):
    import onetile_cases as oc
    for name, case in (("ide_path7_d8", "burgers_ide-d8-canonical-full"), ("burgers_d4", "burgers-d4-canonical-full"),
                       ("burgers_d6", "burgers-d6-canonical-full"), ("adr_d8", "adr-d8-canonical-full")):
        eng = oc.engine_for(case)
        eng.adam_init(1e-3, 0.9, 0.999, 1e-7)
        adam = eng.adam_run(40)
        eng.lbfgs_begin(60, 0.8, 50, np.finfo(float).eps)
        _, lb, _ = eng.lbfgs_run(60)
        loss, grad, terms = eng.loss_grad()
        d = os.path.join(out, name)
        os.makedirs(d, exist_ok=True)
        for k, v in (("weights", eng.get_weights()), ("adam_losses", adam), ("lbfgs_losses", lb), ("loss", np.float64(loss)),
                     ("loss_terms", terms), ("grad", grad)):
            np.save(os.path.join(d, k + ".npy"), np.asarray(v))
        print("%s: path %d, loss %.17g after %d L-BFGS entries" % (name, eng.kernel_path(), loss, len(lb)))
        eng.close()


def compare(a, b):
    bad = n = 0
    for root, _, files in sorted(os.walk(a)):
        for f in sorted(files):
            if not f.endswith(".npy"):
                continue
            rel = os.path.relpath(os.path.join(root, f), a)
            x, y = np.load(os.path.join(a, rel)), np.load(os.path.join(b, rel))
            same = x.shape == y.shape and np.array_equal(x, y)
            n += 1
            bad += not same
            print("%-40s %-10s %s" % (rel, x.shape, "bit-equal" if same else "DIFFERS (%d values)" % int(np.sum(x != y))))
    print("%d arrays, %d differ" % (n, bad))
    return 1 if bad or not n else 0


if __name__ == "__main__":
    sys.exit(dump(sys.argv[2]) if sys.argv[1] == "dump" else compare(sys.argv[2], sys.argv[3]))
