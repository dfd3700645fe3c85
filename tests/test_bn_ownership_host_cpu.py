"""The named ownership branches of tests/_bn_ownership.py resolve (no GPU): for every kernel, type and stride each
branch has a candidate shape whose plan, as the library reports it, satisfies the branch's predicate, and the resolved
branches are the whole table -- tests/test_gpu_bn_ownership.py runs exactly these.  For the dwbn shapes the float64
reference alone must meet the clip-coverage condition of tests/test_gpu_dwbn.py (some y == 0, some y == 6, some strictly
between): it is a condition on the inputs, met by the choice of the seed."""
import pytest
import torch

import _bn_ownership as B
import _mobilenet_ref as RM
import test_gpu_dwbn as TD

TRAIN = [torch.float32, torch.bfloat16]
ALL = TRAIN + [torch.float16]


def test_every_dwbn_branch_resolves():
    seen = set()
    for name, strides, cands, pred in B.DWBN:
        for stride in strides:
            for dt in ALL:
                i = B.dwbn(name, stride, dt)
                assert pred(i) and (i["shape"], i["layout"]) in cands and i["stride"] == stride, (name, stride, dt)
                assert i["G"] > 1 and i["NB"] == 1, (name, i)                 # every one of them shares a tile
                n, c, h, w = i["shape"]
                assert {k: i[k] for k in ("G", "RB", "NB", "U", "S", "per")} == B.ops.dwbn_plan(n, c, h, w, stride, dt)
                seen.add((name, stride))
                print(f"dwbn {name} | s{stride} {dt}: {i['shape']} {i['layout']} wide={int(i['wide'])} "
                      f"G={i['G']} U={i['U']} S={i['S']} per={i['per']}")
    assert seen == set(B.DWBN_CASES) and len(B.DWBN_CASES) == sum(len(b[1]) for b in B.DWBN)
    assert len({b[0] for b in B.DWBN}) == len(B.DWBN) == 10
    # the branches the table promises, at the shapes it was written for
    i = B.dwbn("wide G>1, whole groups, U a multiple of S", 1, torch.float32)
    assert (i["shape"], i["G"], i["S"]) == ((8, 512, 8, 8), 4, 2)
    assert B.dwbn("wide G>1, whole groups, U a multiple of S", 2, torch.bfloat16)["shape"] == (8, 512, 16, 16)
    i = B.dwbn("G>1, short last group, several groups per workgroup", 1, torch.float32)
    assert (i["G"], i["U"], i["per"]) == (2, 3, 2)
    assert B.dwbn("G limited by the output cap, short last group", 1, torch.float32)["G"] == 8
    assert B.dwbn("G limited by the staged tile, a plane that is all halo", 1, torch.float32)["G"] == 455
    assert B.dwbn("G limited by N / want, MobileNetV2's last stage at batch 128", 1, torch.float32)["G"] == 64
    with pytest.raises(AssertionError, match="no candidate"):
        B._smallest("dwbn", "nothing", [])


@pytest.mark.parametrize("dtype", ALL, ids=["f32", "bf16", "f16"])
def test_dwbn_shapes_cover_both_clamps_in_float64(dtype):
    done = set()
    for name, stride in B.DWBN_CASES:
        shape = B.dwbn(name, stride, dtype)["shape"]
        if (shape, stride) in done:
            continue
        done.add((shape, stride))
        x, w, gamma, beta, _, _, _ = TD.make_inputs(shape, stride, seed=B.dwbn_seed(shape, stride))
        y = RM.stage(x.to(dtype), w, gamma, beta, stride)["y"]
        assert shape[0] * y.shape[2] * y.shape[3] >= 24, shape
        assert int((y == 0).sum()) > 0 and int((y == 6).sum()) > 0 and int(((y > 0) & (y < 6)).sum()) > 0, (shape, stride)


def test_every_bnact_branch_resolves():
    seen = set()
    for name, cands, pred in B.BNACT:
        for dt in ALL:
            i = B.bnact(name, dt)
            assert pred(i) and (i["shape"], i["layout"]) in cands, (name, dt)
            seen.add(name)
            print(f"bnact {name} | {dt}: {i['shape']} vec={i['vec']} S={i['S']} span={i['span']} steps={i['steps']} "
                  f"step_q={i['step_q']} step_r={i['step_r']} wraps={i['wraps']}")
    assert seen == {b[0] for b in B.BNACT} and len(seen) == len(B.BNACT) == 3
    i = B.bnact(B.BNACT[0][0], torch.float32)
    assert (i["shape"], i["M"], i["steps"], i["step_q"], i["step_r"]) == ((8, 3, 7, 7), 392, 2, 5, 11)
    i = B.bnact(B.BNACT[1][0], torch.float32)                                  # ResNet-50 layer4-like planes
    assert (i["S"], i["steps"], i["step_q"], i["step_r"]) == (1, 3, 7, 16)
    i = B.bnact(B.BNACT[1][0], torch.bfloat16)
    assert (i["shape"], i["S"], i["steps"], i["step_q"], i["step_r"]) == ((16, 2048, 12, 12), 1, 2, 14, 32)
    # at 15 images the second 16-bit trip holds only lanes that have not wrapped: a walk that forgot the wrap would pass
    assert B.bnact_info((15, 2048, 12, 12), "plain", torch.bfloat16)["wraps"] == 0 and i["wraps"] > 0
    assert B.bnact(B.BNACT[2][0], torch.float32)["shape"] == (17, 2048, 8, 8)
    assert B.bnact(B.BNACT[2][0], torch.bfloat16)["shape"] == (33, 2048, 8, 8)
    # the 7x7 planes of ResNet-50's layer4: one step at batch 2 (what tests/test_gpu_bnact.py runs), the walk from 6 on
    assert B.bnact_info((2, 2048, 7, 7), "plain", torch.float32)["steps"] == 1
    i = B.bnact_info((6, 2048, 7, 7), "plain", torch.float32)
    assert (i["vec"], i["steps"], i["step_q"], i["step_r"]) == (1, 2, 5, 11)


def test_every_densebn_branch_resolves():
    seen = set()
    for name, cands, pred in B.DENSEBN:
        for dt in ALL:
            i = B.densebn(name, dt)
            assert pred(i) and i["layout"] in cands, (name, dt)
            seen.add(name)
            print(f"densebn {name} | {dt}: {i['layout']} vec={i['vec']} S={i['S']} span={i['span']} steps={i['steps']} "
                  f"step_q={i['step_q']} step_r={i['step_r']} wraps={i['wraps']} stats={[(s['S'], s['span']) for s in i['stats']]}")
    assert seen == {b[0] for b in B.DENSEBN} and len(seen) == len(B.DENSEBN) == 4
    assert set(B.DENSEBN_EVAL_AND_F16) <= seen
    i = B.densebn(B.DENSEBN[2][0], torch.float32)
    assert (i["S"], i["span"]) == (1, 3072) and [(s["S"], s["span"]) for s in i["stats"]] == [(2, 2048), (3, 1024), (3, 1024)]
    assert B.densebn(B.DENSEBN[2][0], torch.bfloat16)["layout"][1] == 16 and i["layout"][1] == 15
    assert B.densebn_info(((8, 4, 4), 6, 6, 8, 1), torch.float32)["wraps"] == 0         # 288 values: no lane goes on
    assert B.densebn(B.DENSEBN[3][0], torch.float32)["layout"][1] == 65
    assert B.densebn(B.DENSEBN[3][0], torch.bfloat16)["layout"][1] == 130
