#!/usr/bin/env python3
"""Which kernels run when an operand is off the 16-byte grid.

    python tools/alignment_trace.py --out DIR      # every group below in a child process of its own under
                                                   # rocprofv3 --kernel-trace --stats (no counters); DIR/summary.txt
    python tools/alignment_trace.py --group NAME   # one group, untraced (what the children run)

Every call of a group has at least one operand 1, 2 or 3 elements off the grid (the wide-tile group says which), at
widths that are multiples of 4, so that a `<1>` / scalar kernel in the list was chosen by the pointer and not by k.  The
calls are those of tests/test_alignment_gpu.py (its _check_spmm holds each to the oracle as it runs); the SDDMM group
leaves out that test's aligned run."""
import argparse
import csv
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _spmm_unsliced(T):
    adj = T._adj(T._graph("long"))
    for k in (8, 16, 64, 128):
        for epilogue in (False, True):
            for which in T._sets(epilogue):
                T._check_spmm(adj, "long", k, which, 1, epilogue)


def _wide_tile(T, tile, cases):
    adj = T._adj(T._graph("long"))
    adj.set_gather_width(1)
    adj.set_tile_cols(tile)
    for which, off in cases:
        T._check_spmm(adj, "long", 256, which, off, True)


def _ragged(T):
    adj = T._adj(T._graph("ragged"), chunk_nnz=64)
    for k in (16, 64):
        T._check_spmm(adj, "ragged", k, "C", 1, True)
        T._check_spmm(adj, "ragged", k, "bias", 1, True)


def _sliced(T, plan, which):
    name = "sym" if plan == "value_free" else "sym_random"
    adj = T._adj(T._graph(name), slices=4, mutable_values=plan == "mutable")
    for k in (64, 512):
        T._check_spmm(adj, name, k, which, 1, True)


def _panels(T, name):
    adj = T._adj(T._graph(name), panels=1)
    for which in ("B", "C"):
        T._check_spmm(adj, name, 64, which, 1, True)


def _bf16(T, cases):
    import torch
    g = T._graph("bf16")
    adj = T._adj(g, symmetric=True, slices=4)
    B = torch.randn((g[4], 128), generator=torch.Generator().manual_seed(128)).to(T.BF16)
    for ob, cdtype, oc in cases:
        Bv, _ = T.offset_view(B, ob, T.BF16, T.DEV)
        out, _ = T.offset_view((adj.m, 128), oc, cdtype, T.DEV)
        adj.matmul_raw(Bv, out=out)
    torch.cuda.synchronize()


def _sddmm(T, slices):
    import numpy as np
    import torch
    g = T._graph("rect")
    adj = T._adj(g, slices=slices)
    rng = np.random.default_rng(64)
    A = rng.standard_normal((g[3], 64)).astype(np.float32)
    B = rng.standard_normal((g[4], 64)).astype(np.float32)
    ref, mag = T.sddmm_ref(g[0], g[1], A, B, T.DEV)
    for oa, ob in ((1, 0), (0, 1), (2, 3)):
        Av, _ = T.offset_view(A, oa, T.F32, T.DEV)
        Bv, _ = T.offset_view(B, ob, T.F32, T.DEV)
        T.check_sddmm(adj.sddmm(Av, Bv), ref, mag)
    torch.cuda.synchronize()


def _gather_rows(T):
    import numpy as np
    import torch
    import gcn_amd
    src = np.random.default_rng(0).standard_normal((777, 64)).astype(np.float32)
    idx = np.arange(0, 777, 3, dtype=np.int32)
    for os_, od in ((1, 0), (0, 1)):
        sv, _ = T.offset_view(src, os_, T.F32, T.DEV)
        out, _ = T.offset_view((len(idx), 64), od, T.F32, T.DEV)
        gcn_amd.gather_rows(sv, torch.from_numpy(idx).to(T.DEV), out=out)
    torch.cuda.synchronize()


GROUPS = {
    "unsliced, k in 8 16 64 128, B / C / bias / all at 1 float": _spmm_unsliced,
    "tile 256, gather width 1, k 256: bias alone at 1 float (B, C aligned)": lambda T: _wide_tile(T, 256, [("bias", 1)]),
    "tile 256, gather width 1, k 256: B at 2 floats": lambda T: _wide_tile(T, 256, [("B", 2)]),
    "tile 256, gather width 1, k 256: B at 1 float": lambda T: _wide_tile(T, 256, [("B", 1)]),
    "tile 128, gather width 1, k 256: bias alone at 1 float (B, C aligned)": lambda T: _wide_tile(T, 128, [("bias", 1)]),
    "tile 128, gather width 1, k 256: C at 1 float": lambda T: _wide_tile(T, 128, [("C", 1)]),
    "ragged matrix (empty rows, cut rows), bias + ReLU, C or bias at 1 float": _ragged,
    "4 slices, value-free, k in 64 512: B at 1 float": lambda T: _sliced(T, "value_free", "B"),
    "4 slices, value-free, k in 64 512: C at 1 float": lambda T: _sliced(T, "value_free", "C"),
    "4 slices, mutable values, k in 64 512: B at 1 float": lambda T: _sliced(T, "mutable", "B"),
    "4 slices, values that do not factor, k in 64 512: all at 1 float": lambda T: _sliced(T, "virtual_csr", "all"),
    "LDS-staged panels, k 64: B, then C, at 1 float": lambda T: _panels(T, "banded"),
    "dense MFMA panels, k 64: B, then C, at 1 float": lambda T: _panels(T, "dense_band"),
    "bf16 hot path, k 128: B at 1, 2, 4 halves (bf16 C aligned)": lambda T: _bf16(T, [(o, T.BF16, 0) for o in (1, 2, 4)]),
    "bf16 hot path, k 128: bf16 C at 1 half": lambda T: _bf16(T, [(0, T.BF16, 1)]),
    "bf16 hot path, k 128: bf16 C at 4 halves": lambda T: _bf16(T, [(0, T.BF16, 4)]),
    "bf16 hot path, k 128: fp32 C at 1 float": lambda T: _bf16(T, [(0, T.F32, 1)]),
    "SDDMM, unsliced plan, k 64: A, B, both off the grid": lambda T: _sddmm(T, 0),
    "SDDMM, 4 slices, k 64: A, B, both off the grid": lambda T: _sddmm(T, 4),
    "gather_rows, k 64: source, then destination, at 1 float": _gather_rows,
}


def _run_group(name):
    import test_alignment_gpu as T
    GROUPS[name](T)


def _trace_all(out):
    os.makedirs(out, exist_ok=True)
    lines = ["kernels of libgcnspmm.so per group of misaligned calls: rocprofv3 --kernel-trace --stats, one process per group",
             "(tools/alignment_trace.py; calls, kernel name).  Plan construction runs in the same process: its kernels are",
             "listed too.", ""]
    for i, name in enumerate(GROUPS):
        d = os.path.join(out, f"g{i:02d}")
        cmd = ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d,
               "--", sys.executable, os.path.abspath(__file__), "--group", name]
        with open(os.path.join(out, f"g{i:02d}.log"), "w") as log:
            rc = subprocess.run(cmd, stdout=log, stderr=subprocess.STDOUT).returncode
        if rc != 0:                                       # nothing more on the GPU after a failure
            sys.exit(f"group {name!r} ended with status {rc}: see {d}.log")
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        assert len(stats) == 1, stats
        rows = [(r["Name"], int(r["Calls"])) for r in csv.DictReader(open(stats[0])) if "gcn::" in r["Name"]]
        lines.append(f"== {name}")
        lines += [f"{calls:6d}  {kern}" for kern, calls in sorted(rows)]
        lines.append("")
        print(lines[-len(rows) - 2], len(rows), "kernels", flush=True)
    with open(os.path.join(out, "summary.txt"), "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--group", choices=list(GROUPS))
    a = ap.parse_args()
    if a.group:
        _run_group(a.group)
    elif a.out:
        _trace_all(a.out)
    else:
        ap.error("--out DIR or --group NAME")
