"""The staged stream loads of the four-engine group walk (group_walk.h): the value-free walk fetches the stream words of a
STAGE of runs (64 entries each) together, at the chunk's start and again wherever a stage ends inside the chunk.  The
chunk length T of a real plan is 256..1024 and a small graph never gets a long one, so every case runs in a child process
with GCN_AMD_GROUP_T=<T> (read once per process, plan_policy.cpp): T = 64 is one run, 192 a partial first stage, 256 and
512 exactly one stage of 4 and of 8 runs, 320, 576 and 1024 one or two stages and a remainder (or none) for both stage
lengths.  Each child checks, on a graph with a hub row that spans several chunks (and several stages at small T), empty
rows and one-entry rows, with 2 and 5 slices:
  * value-free fp32, exact: integer features, values u[r]*u[c] with u = 2^-e — the result EQUALS the fp64 oracle
    (k = 64, 128 and 200: the last 64-column tile partial);
  * value-free fp32, random normal features: max|C - C*| / max|C*| <= 1e-5, plain and with bias + ReLU;
  * bf16 tables (k = 128, 320) through the same walk, within the bound of test_bf16_gpu.py;
  * a weighted plan (the walk's other branch: unchanged, but the same template) within 1e-5;
and asserts the kernel each call names, so that no case passes on another route.  The parent also compares the digests
the children print for the random-normal result: a row cut by chunk ends is summed piece by piece, so another T gives other
last bits — seven different digests say that the forced length reached the plans."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gcn_amd
from util import (assert_exact, assert_exact_inputs, bf16_assert_bound, bf16_reference, factored_values, int_features,
                  oracle_spmm, pow2_factors, rel_err)

pytestmark = pytest.mark.gpu
TOL = 1e-5
CHUNK_LENGTHS = (64, 192, 256, 320, 512, 576, 1024)
N, DEGREE, HUB, HUB_LEN = 3001, 50, 1234, 3000


def _graph():
    """n = 3001 (odd), about 50 entries per row — a plan runs value-free from 48 stored entries per column on
    (kVallessMinPerCol, plan_policy.h); with fewer, the factors are kept but the weighted kernel runs; row HUB holds 3000;
    rows 5, 6 and the last are empty, rows 9, 10, 11 hold one entry each.  u = 2^-e factors."""
    rng = np.random.default_rng(77)
    rows = np.repeat(np.arange(N), DEGREE)
    cols = rng.integers(0, N, N * DEGREE)
    keep = ~np.isin(rows, [5, 6, N - 1, 9, 10, 11, HUB])
    rows, cols = rows[keep], cols[keep]
    rows = np.concatenate([rows, [9, 10, 11], np.full(HUB_LEN, HUB)])
    cols = np.concatenate([cols, [0, N - 1, 1500], rng.choice(N, HUB_LEN, replace=False)])
    key = np.unique(rows.astype(np.int64) * N + cols)            # sorted by (row, column), no repeated entries
    rows, cols = (key // N).astype(np.int64), (key % N).astype(np.int32)
    rp = np.zeros(N + 1, np.int64)
    np.add.at(rp, rows + 1, 1)
    rp = np.cumsum(rp).astype(np.int32)
    lens = np.diff(rp)
    assert lens[HUB] == HUB_LEN and (lens == 0).sum() == 3 and (lens == 1).sum() >= 3 and len(cols) // N >= 48
    u = pow2_factors(N, 5)
    return rp, cols, factored_values(rp, cols, u, u), u


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


def _stage_child():
    rp, ci, va, u = _graph()
    digest = hashlib.sha256()
    for S in (2, 5):
        adj = gcn_amd.CsrAdjacency(_t(rp), _t(ci), _t(va), (N, N), slices=S)
        adj.set_value_factors(_t(u), _t(u))
        assert adj.num_slices == S and adj.has_value_factors
        # exact: every partial sum is an fp32 number in any order
        for k in (64, 128, 200):
            assert adj.main_kernel(k).startswith("gcn::spmm_group_ring_kernel<"), adj.main_kernel(k)
            B = int_features(N, k, seed=300 + k)
            assert_exact_inputs(rp, ci, va, B)
            out = torch.full((N, k), float("nan"), device="cuda:0")
            C = adj.matmul_raw(_t(B), out=out).cpu().numpy()
            assert_exact(C, oracle_spmm(rp, ci, va, B), f"exact S={S} k={k}")
            assert np.all(C[np.diff(rp) == 0] == 0.0)
        # random normal features, plain and with the fused epilogue
        k = 128
        rng = np.random.default_rng(400 + S)
        B = rng.standard_normal((N, k)).astype(np.float32)
        ref = oracle_spmm(rp, ci, va, B)
        C = adj.matmul_raw(_t(B)).cpu().numpy()
        err = rel_err(C, ref)
        print(f"S={S} fp32 rel err {err:.2e}")
        assert err <= TOL, (S, err)
        digest.update(C[HUB].tobytes())
        bias = rng.standard_normal(k).astype(np.float32)
        Ce = adj.matmul_raw(_t(B), bias=_t(bias), relu=True).cpu().numpy()
        err = rel_err(Ce, np.maximum(ref + bias, 0))
        print(f"S={S} fp32 bias+relu rel err {err:.2e}")
        assert err <= TOL, (S, err)
        # bf16 tables: one and three tiles of 128 columns (the last one half full)
        for k in (128, 320):
            name = adj.main_kernel(k, dtype=torch.bfloat16)
            assert name.startswith("gcn::spmm_group_bf16_kernel<"), name
            B16 = _t(np.random.default_rng(500 + k).standard_normal((N, k)).astype(np.float32), torch.bfloat16)
            Cref, absref = bf16_reference(rp, ci, va, B16)
            bf16_assert_bound(adj.matmul_raw(B16), Cref, absref, bf16_out=True)
        # the weighted walk: a plan told to forget its factors
        wadj = gcn_amd.CsrAdjacency(_t(rp), _t(ci), _t(va), (N, N), slices=S)
        wadj.plan                                                    # noqa: B018  (builds the plan)
        wadj.set_value_factors(None, None)
        assert not wadj.has_value_factors
        assert wadj.main_kernel(128).startswith("gcn::spmm_group_weighted_kernel<"), wadj.main_kernel(128)
        err = rel_err(wadj.matmul_raw(_t(B)).cpu().numpy(), ref)
        print(f"S={S} weighted rel err {err:.2e}")
        assert err <= TOL, (S, err)
    print("stage digest", digest.hexdigest())


_DIGESTS = {}


def _run_child(T):
    """the child's digest for chunk length T (one child per T and session)"""
    if T not in _DIGESTS:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = dict(os.environ, GCN_AMD_GROUP_T=str(T), PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--stage-child"], env=env, capture_output=True,
                             text=True, timeout=600, cwd=os.path.dirname(os.path.abspath(__file__)))
        print(out.stdout)
        assert out.returncode == 0 and "stage digest" in out.stdout, out.stdout[-1500:] + out.stderr[-1500:]
        _DIGESTS[T] = out.stdout.split("stage digest")[1].split()[0]
    return _DIGESTS[T]


@pytest.mark.parametrize("T", CHUNK_LENGTHS)
def test_staged_stream_loads_at_chunk_length(T):
    _run_child(T)


def test_forced_chunk_length_reaches_the_plans():
    """every chunk length cut the hub row elsewhere"""
    digests = {T: _run_child(T) for T in CHUNK_LENGTHS}
    assert len(set(digests.values())) == len(CHUNK_LENGTHS), digests


if __name__ == "__main__":
    if "--stage-child" in sys.argv:
        _stage_child()
