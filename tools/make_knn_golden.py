#!/usr/bin/env python3
"""tests/golden/knn_hypergraph_*.npz: inputs and the outputs of the reference's own hypergraph construction on them.

    python tools/make_knn_golden.py --reference DIR        # DIR holds the reference tree (pyhgnn/utils/hypergraph_utils.py)

Runs on the CPU.  For every case: x (fp32-representable Gaussians), H = construct_H_with_KNN_from_distance(Eu_dis(x), k) and
G = generate_G_from_H(H), all computed by the reference's functions in fp64.  The fixtures are data only.
The reference's ``np.mat`` is gone from numpy 2: this process sets ``np.mat = np.asmatrix`` before importing it.  Its
``hyperedge_concat`` does not run under numpy 2 either and is not called (a single k needs no concatenation).
An input is REFUSED when, for some centre, the relative gap between the distances of the (k-1)-th and the k-th nearest other
vertex is below 1e-4: the reference's fp64 norm-form distances and any other arithmetic then need not agree on the set, and a
comparison would hinge on rounding."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(200, 16, 10, 186), (130, 40, 10, 62), (150, 3, 5, 45)]          # (n, d, k, default_rng seed)
MIN_GAP = 1e-4


def smallest_gap(x, k):
    """min over centres of (d_k - d_{k-1}) / d_k, d_t the distance to the t-th nearest other vertex (fp64, difference form)"""
    x = x.astype(np.float64)
    gap = np.inf
    for c in range(x.shape[0]):
        d = np.sqrt(((x - x[c]) ** 2).sum(axis=1))
        d = np.sort(np.delete(d, c))
        gap = min(gap, (d[k - 1] - d[k - 2]) / d[k - 1])
    return gap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory of the reference tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    np.mat = np.asmatrix
    sys.path.insert(0, os.path.join(args.reference, "pyhgnn"))
    from utils.hypergraph_utils import Eu_dis, construct_H_with_KNN_from_distance, generate_G_from_H
    for n, d, k, seed in CASES:
        x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
        gap = smallest_gap(x, k)
        if gap < MIN_GAP:
            sys.exit(f"(n, d, k, seed) = {(n, d, k, seed)}: smallest gap {gap:.3g} < {MIN_GAP}: choose another seed")
        H = np.asarray(construct_H_with_KNN_from_distance(Eu_dis(x.astype(np.float64)), k, True, 1))
        G = np.asarray(generate_G_from_H(H))
        path = os.path.join(args.out, f"knn_hypergraph_n{n}_d{d}_k{k}.npz")
        np.savez_compressed(path, x=x, k=np.int64(k), seed=np.int64(seed), gap=np.float64(gap), H=H, G=G)
        print(f"{os.path.relpath(path, ROOT)}: smallest gap {gap:.3g}, {int((H != 0).sum())} entries of H, "
              f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
