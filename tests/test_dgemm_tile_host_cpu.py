"""What `tadmm_dgemm_tile_f64` (the test entry that launches the filter's tile product and daxpby) refuses, through the
host-only `tadmm_dgemm_tile_check`: no device is needed, the pointers are never followed."""
import ctypes as C

import pytest

PTR = 0x1000        # any non-null value


def _prob(**kw):
    from tadmm._cabi import DgemmTileProb
    q = DgemmTileProb()
    q.A, q.B, q.C = PTR, PTR, PTR
    q.selA = q.selB = q.selC = q.selP = q.selQ = -1
    q.M, q.N, q.K, q.lda, q.ldb, q.ldc, q.mode = 64, 96, 32, 32, 32, 96, 0
    for k, v in kw.items():
        if k == "ring":
            q.ring[0], q.ring[1], q.ring[2] = v
        else:
            setattr(q, k, v)
    return q


def _check(q, tile=(32, 32), axpby=0, nprob=1):
    from tadmm import _cabi
    return _cabi.load().tadmm_dgemm_tile_check(nprob, C.byref(q), tile[0], tile[1], axpby)


def test_binding_matches_the_library_struct():
    from tadmm import _cabi
    assert _cabi.load().tadmm_dgemm_tile_prob_bytes() == C.sizeof(_cabi.DgemmTileProb)


@pytest.mark.parametrize("tile", [(32, 32), (64, 32), (64, 64)])
def test_accepts_every_tile_and_mode(tile):
    assert _check(_prob(), tile) == 0
    assert _check(_prob(mode=1, P=PTR, coef=PTR), tile) == 0
    assert _check(_prob(mode=1, P=PTR, Q=PTR, coef=PTR), tile) == 0
    assert _check(_prob(mode=2, P=PTR, rowpart=PTR), tile) == 0
    assert _check(_prob(mode=3, P=PTR, theta=PTR, rowpart=PTR), tile) == 0
    ring = (PTR, PTR, PTR)
    assert _check(_prob(A=None, C=None, ring=ring, selA=1, selP=1, selQ=0, selC=2, mode=1, coef=PTR, N=32, ldc=32), tile) == 0
    assert _check(_prob(A=None, B=None, P=PTR, coef=PTR), tile, axpby=1) == 0


@pytest.mark.parametrize("why,kw", [
    ("M not a multiple of 32", dict(M=48)), ("N not a multiple of 32", dict(N=80)), ("K not a multiple of 32", dict(K=48)),
    ("M = 0", dict(M=0)), ("negative K", dict(K=-32)),
    ("odd lda", dict(lda=33)), ("lda < K", dict(K=64)), ("ldb < K", dict(K=64, lda=64)), ("ldc < N", dict(ldc=64)),
    ("mode 4", dict(mode=4)), ("mode -1", dict(mode=-1)),
    ("no A", dict(A=None)), ("no B", dict(B=None)), ("no C", dict(C=None)),
    ("selA without a ring", dict(selA=0)), ("selC = 3", dict(selC=3, ring=(PTR, PTR, PTR))),
    ("ring with a hole", dict(selA=0, ring=(PTR, None, PTR))),
    ("mode 1 without P", dict(mode=1, coef=PTR)), ("mode 1 without coef", dict(mode=1, P=PTR)),
    ("selQ without a ring", dict(mode=1, P=PTR, coef=PTR, selQ=0)),
    ("mode 2 without rowpart", dict(mode=2, P=PTR)), ("mode 3 without theta", dict(mode=3, P=PTR, rowpart=PTR)),
])
def test_refuses(why, kw):
    assert _check(_prob(**kw)) == -1, why


def test_refuses_unknown_tiles_counts_and_axpby_without_operands():
    q = _prob()
    for tile in [(32, 64), (64, 16), (16, 16), (0, 0), (128, 64)]:
        assert _check(q, tile) == -1, tile
    assert _check(q, nprob=0) == -1
    assert _check(q, nprob=65) == -1
    from tadmm import _cabi
    assert _cabi.load().tadmm_dgemm_tile_check(1, None, 32, 32, 0) == -1
    assert _check(_prob(), axpby=1) == -1                       # no P, no coef
    assert _check(_prob(P=PTR), axpby=1) == -1                  # no coef
    assert _check(_prob(P=PTR, coef=PTR, C=None), axpby=1) == -1
