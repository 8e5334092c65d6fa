"""ln L of four small seeded fits, written to an .npy, to compare two builds of the engine byte for byte: run it once per build
(VAG_LIB_PATH selects the library) in the same visit and compare the files with --compare.

The fits are those of tests/test_loglike_entry_points.py: (a) the 60 C4 point rows alone; (b) one fitter with a point block, a band
group, a centroid group, a visibility group, a degree-polarization group with a limit epoch, limit rows, a noise group with a
calibration term, a counts group and a spectral-index group; (c) the same plus a count-spectrum group with a cross-section, a
template on point rows and two correlated groups (2 and 65 rows): every spec block the likelihood has.  Each is evaluated with 3
walkers (no ordering) and with 64 (the smallest batch evaluated in cost order), twice: the second call runs in the order the first
one left.  (d) the nine fitters of fixture (d) -- (c), (c) plus a second group of one list kind for each of the seven kinds, (c) plus
all seven -- with 3 walkers, once each.  The array is the twelve results of (a) - (c) in that order, concatenated (3 x (3 + 3 + 64 +
64) = 402 values), then the nine of (d) (27 values).  The data of the fits are made by model calls of the build under test, so a
difference may come from the model requests as well as from the likelihood.

    VAG_LIB_PATH=a.so python profiles/loglike_bits.py --out a.npy
    VAG_LIB_PATH=b.so python profiles/loglike_bits.py --out b.npy
    python profiles/loglike_bits.py --compare a.npy b.npy"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def evaluate():
    import test_loglike_entry_points as ep  # noqa: E402
    out = []
    for fixture, walkers in ((ep.fixture_a, ep.walkers_a), (ep.fixture_b, ep.walkers_b), (ep.fixture_c, ep.walkers_c)):
        f, d = fixture()
        for nb in ep.BATCHES:
            th = walkers(nb)
            for _ in range(2):
                out.append(f.loglike_batch(th, d))
    fits, d = ep.fixture_d()
    out += [f.loglike_batch(ep.walkers_c(3), d) for f in fits]
    return np.concatenate(out)


def compare(a, b):
    x, y = np.load(a), np.load(b)
    if x.shape == y.shape and x.tobytes() == y.tobytes():
        print(f"equal: {x.size} values, {np.isfinite(x).sum()} finite")
        return 0
    if x.shape != y.shape:
        print(f"shapes differ: {x.shape} {y.shape}")
        return 1
    diff = np.flatnonzero(x.view(np.uint64) != y.view(np.uint64))
    print(f"differ at {diff.size} of {x.size} indices: {diff.tolist()}")
    for i in diff[:16]:
        print(f"  [{i}] {x[i]!r} {y[i]!r}")
    return 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write ln L to this .npy")
    ap.add_argument("--compare", nargs=2, metavar="NPY", help="compare two files written with --out")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    ll = evaluate()
    print(f"{ll.size} values, {np.isfinite(ll).sum()} finite, library {os.environ.get('VAG_LIB_PATH', '(the product library)')}", flush=True)
    if args.out:
        np.save(args.out, ll)


if __name__ == "__main__":
    main()
