"""The XCD-aware block order of the filter's tile products (`tile_map_build`, csrc/host.h) only permutes independent
tiles: every output byte of `dgemm_nt_tile_kernel`, and of a filtered `ProjectionPlan`, must equal what the same build
gives in plain problem-major order (TADMM_XCD_MAP=0, read whenever a map is built).  The plain order itself is held to
recorded bytes and to float64 by tests/test_gpu_filter_chain_bits.py."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_golden_filter_bits", os.path.join(_GOLDEN, "make_golden_filter_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

TILES = [(32, 32), (64, 32), (64, 64)]
GROUPED = [(96, 160), (64, 96)]          # (M, N) with K = N, one grouped launch, one of the two gated off
ALONE = [(160, 160)]
COEF = (-0.5, -0.75, 0.375)
ENV = ("TADMM_XCD_MAP", "TADMM_TILE_MAP", "TADMM_TILE_MAP_LONGEST")


@pytest.fixture(scope="module")
def operands():
    """Seeded host operands per problem shape, made once: G (N, N), three ring images (M, N), theta (M,)."""
    rng = np.random.default_rng(20240611)
    out = {}
    for M, N in GROUPED + ALONE:
        out[(M, N)] = (bits._grid(rng.standard_normal((N, N))), [bits._grid(rng.standard_normal((M, N))) for _ in range(3)],
                       bits._grid(rng.standard_normal(M)))
    return out


def _launch(operands, shapes, gated, tile, mode, rot):
    """One grouped launch as the filter's recurrence names its operands (A = P = slot rot + 1, Q = slot rot, C = slot
    rot + 2, B = G); returns every byte a problem could have written: its three ring images and its row partials."""
    import torch
    from tadmm import ops
    tile_m, tile_n = tile
    probs, keep = [], []
    for i, (M, N) in enumerate(shapes):
        G, slots, th = operands[(M, N)]
        ring = [bits._dev(s) for s in slots]
        rowpart = torch.full(((N + tile_n - 1) // tile_n, M), 7.0, dtype=torch.float64, device="cuda:0")
        gate = bits._dev(np.array([1 if i == gated else 2], dtype=np.int32))
        probs.append(dict(B=bits._dev(G), ring=ring, rot=bits._dev(np.array([rot], dtype=np.int32)), selA=1, selP=1, selQ=0,
                          selC=2, M=M, N=N, K=N, ldb=N, mode=mode, coef=bits._dev(np.array(COEF)), theta=bits._dev(th),
                          rowpart=rowpart, gate=gate, gate_min=2))
        keep.append((ring, rowpart))
    ops.dgemm_tile(probs, tile_m, tile_n)
    return [[r.cpu().numpy() for r in ring] + [rowpart.cpu().numpy()] for ring, rowpart in keep]


@pytest.mark.parametrize("rot", [0, 1, 2])
@pytest.mark.parametrize("tile", TILES)
def test_tile_product_bytes_do_not_depend_on_the_block_order(operands, monkeypatch, tile, rot):
    from tadmm import ops
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    m, _, _ = ops.tile_map([(160, 160, 160, 32, 32)])
    assert m != [(0, b) for b in range(25)], "the default order is the plain one: nothing is compared"
    for shapes, gated in ((GROUPED, rot % 2), (ALONE, -1)):
        for mode in range(4):
            monkeypatch.delenv("TADMM_XCD_MAP", raising=False)
            new = _launch(operands, shapes, gated, tile, mode, rot)
            monkeypatch.setenv("TADMM_XCD_MAP", "0")
            plain = _launch(operands, shapes, gated, tile, mode, rot)
            for i, (a, b) in enumerate(zip(new, plain)):
                what = "tile %s mode %d rot %d problem %d of %s" % (tile, mode, rot, i, shapes)
                for x, y in zip(a, b):
                    assert x.tobytes() == y.tobytes(), what
                slots = operands[shapes[i]][1]
                touched = any(a[k].tobytes() != slots[k].tobytes() for k in range(3)) or bool(np.any(a[3] != 7.0))
                assert touched == (i != gated), what + (": a gated problem wrote" if i == gated else ": nothing was written")


def _run_plan(table):
    import torch
    from tadmm import ops
    from tadmm._cabi import KIND_TT_LINEAR
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    layers = []
    for shape, tts, ranks in table:
        w = torch.from_numpy((0.1 * rng.standard_normal(shape)).astype(np.float32)).to(dev)
        layers.append(dict(kind=KIND_TT_LINEAR, W=w, U=torch.zeros_like(w), Z=torch.zeros_like(w), tt_shapes=tts, ranks=ranks))
    plan = ops.ProjectionPlan(layers)           # the maps are built here, under the caller's environment
    out, stats = [], []
    for _ in range(2):
        r = plan.run(update_u=True)
        torch.cuda.synchronize()
        out.append(r.detach().cpu().numpy().tobytes())
        stats.append(plan.filter_stats())
    for L in layers:
        out += [L["Z"].cpu().numpy().tobytes(), L["U"].cpu().numpy().tobytes()]
    plan.close()
    return out, stats


@pytest.mark.parametrize("env", [{"TADMM_XCD_MAP": "0"}, {"TADMM_TILE_MAP": "2"}, {"TADMM_TILE_MAP_LONGEST": "0"}])
def test_filtered_plan_is_byte_equal_in_every_order(monkeypatch, env):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    new, new_stats = _run_plan(bits.PLAN_TWO)
    assert new_stats[0]["solves"] > 0 and new_stats[0]["solves"] == new_stats[0]["eligible"], new_stats
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    other, other_stats = _run_plan(bits.PLAN_TWO)
    assert new_stats == other_stats
    assert new == other, "residuals, Z or U differ between the block orders"
