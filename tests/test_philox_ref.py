"""The numpy reference of the dropout mask (util.philox4x32_10, util.dropout_keep) against the Random123 known-answer
vectors of Philox4x32-10 and the threshold's edge values: the GPU tests compare every carrier of the mask with it."""
import numpy as np
import pytest

from util import dropout_keep, dropout_threshold, philox4x32_10

KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answer_vectors(ctr, key, want):
    got = philox4x32_10(ctr, key)
    assert tuple(int(w) for w in got) == want


def test_vectorised_calls_match_scalar_ones():
    ctrs = np.array([k[0] for k in KAT], dtype=np.uint64).T
    keys = np.array([k[1] for k in KAT], dtype=np.uint64).T
    got = np.stack(philox4x32_10(tuple(ctrs), tuple(keys)), axis=1)
    assert got.tolist() == [list(k[2]) for k in KAT]


def test_threshold_edges():
    assert dropout_threshold(2.0 ** -33) == 0
    assert dropout_threshold(2.0 ** -32) == 1
    assert dropout_threshold(np.nextafter(np.float32(1), np.float32(0))) == 0xFFFFFF00
    assert dropout_threshold(0.5) == 0x80000000
    assert dropout_threshold(0.3) == int(np.floor(float(np.float32(0.3)) * 2.0 ** 32))   # the float32 the ABI receives
    assert dropout_keep(4097, 2.0 ** -33, 5, 9).all()                    # threshold 0: everything is kept


def test_dropout_keep_uses_the_documented_counter_and_key():
    seed, offset = 0x9E3779B97F4A7C15, 2 ** 40 + 3
    count, p = 23, 0.5
    keep = dropout_keep(count, p, seed, offset)
    assert keep.shape == (count,) and keep.dtype == bool
    for i in (0, 1, 2, 3, 4, 7, 21, 22):
        w = philox4x32_10((i // 4, 0, offset & 0xFFFFFFFF, offset >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        assert keep[i] == (int(w[i % 4]) >= 0x80000000)
    # the words of the zero counter and key are the first known-answer vector: 66.., e1.., bc.., 9b.. are all >= 2^31
    # except the first
    assert dropout_keep(4, 0.5, 0, 0).tolist() == [False, True, True, True]
    # 64-bit seeds and offsets are not truncated; the high counter word (element index >= 2^34) enters as c1
    assert not np.array_equal(dropout_keep(256, 0.5, 2 ** 32, 0), dropout_keep(256, 0.5, 0, 0))
    assert not np.array_equal(dropout_keep(256, 0.5, 0, 2 ** 32), dropout_keep(256, 0.5, 0, 0))
    hi = philox4x32_10((0, 1, 0, 0), (0, 0))
    assert tuple(int(w) for w in hi) != KAT[0][2]


def test_drop_rate():
    keep = dropout_keep(1 << 16, 0.3, 42, 7)
    assert abs((~keep).mean() - 0.3) < 0.01
