"""The ownership branches of the three fused BatchNorm launches, by name (no GPU needed to resolve them).

csrc/bnact.hip, csrc/dwbn.hip and csrc/densebn.hip derive from the shape alone how a channel's values are cut into
splits, bands and groups of images and how a workgroup walks what it owns.  Each table below names the branches of one
kernel: (name, [strides,] candidate shapes, predicate).  `dwbn`, `bnact` and `densebn` return the smallest candidate
whose plan -- asked of the library through `ops.dwbn_plan`, `ops.bnact_plan` and `ops.densebn_plan`, not restated --
satisfies the predicate, with the plan and what the predicate looked at, and raise when none does: a change of a planner
that moves a shape off its branch fails tests/test_bn_ownership_host_cpu.py instead of silently testing something else.

The access width is chosen by construction: 16 bytes of elements (VEC = 4 float32, 8 sixteen-bit) when every base is
16-byte aligned (layout "plain") and the width rule of the kernel holds, one element when the tensor is placed one
element past a 16-byte boundary (layout "odd") or the width is no whole number of 16-byte units.

The constants the predicates use are those include/tadmm.h documents: a staged dwbn tile of 4096 floats and at most 2048
outputs, 1024 workgroups aimed at (dwbn); trips of 256 lanes times VEC (bnact, densebn)."""
import torch

from tadmm import ops

ES = {torch.float32: 4, torch.bfloat16: 2, torch.float16: 2}
DW_TILE, DW_TILE_OUT, DW_TARGET = 4096, 2048, 1024


def lanes(dtype):
    """Elements of a 16-byte access."""
    return 16 // ES[dtype]


def numel(shape):
    n = 1
    for v in shape:
        n *= v
    return n


def _smallest(kernel, name, found):
    if not found:
        raise AssertionError(f"{kernel}: no candidate shape takes the branch {name!r}")
    return min(found, key=lambda case: case["numel"])


# ------------------------------------------------------------------------------------------------------------ dwbn
def dwbn_info(shape, layout, stride, dtype):
    """The plan of a dwbn shape and everything a predicate may look at."""
    n, c, h, w = shape
    ho, wo = ops.dwbn_out_hw(h, w, stride)
    v = lanes(dtype)
    i = dict(ops.dwbn_plan(n, c, h, w, stride, dtype))
    width_ok = w % v == 0 and wo % v == 0
    i.update(N=n, C=c, H=h, W=w, Ho=ho, Wo=wo, stride=stride, dtype=dtype, layout=layout, width_ok=width_ok,
             wide=width_ok and layout == "plain", want=max(1, -(-DW_TARGET // c)))
    return i


def _dw_fits_tile(i, g):
    """g whole planes with their halos fit the staged input tile and the staged dz tile."""
    rin = (i["Ho"] - 1) * i["stride"] + 3
    return g * rin * (i["W"] + 2) <= DW_TILE and g * (i["Ho"] + 2) * (i["Wo"] + 2) <= DW_TILE


def _dw_fits_out(i, g):
    return g * i["Ho"] * i["Wo"] <= DW_TILE_OUT


# (name, strides, [(shape, layout of x)], predicate on dwbn_info)
DWBN = [
    ("wide G>1, whole groups, U a multiple of S", (1, 2), [((8, 512, 8, 8), "plain"), ((8, 512, 16, 16), "plain")],
     lambda i: i["G"] > 1 and i["wide"] and i["N"] % i["G"] == 0 and i["U"] % i["S"] == 0),
    # 16-byte for float32; for 16-bit elements 16-byte at stride 1 and by element at stride 2 (Wo = 4)
    ("G>1, short last group, several groups per workgroup", (1, 2), [((5, 512, 4, 8), "plain")],
     lambda i: i["G"] > 1 and i["N"] % i["G"] != 0 and i["per"] > 1 and
     i["wide"] == (not (ES[i["dtype"]] == 2 and i["stride"] == 2))),
    ("G>1 by element: the width", (1, 2), [((5, 600, 9, 11), "plain")],
     lambda i: i["G"] > 1 and not i["width_ok"] and i["layout"] == "plain"),
    ("G>1 by element: a misaligned base", (1, 2), [((8, 512, 8, 8), "odd"), ((8, 512, 16, 16), "odd")],
     lambda i: i["G"] > 1 and i["width_ok"] and i["layout"] == "odd" and not i["wide"]),
    ("G == N, one workgroup per channel", (1, 2), [((7, 1024, 4, 4), "plain")],
     lambda i: i["G"] == i["N"] > 1 and i["S"] == 1 and i["U"] == 1),
    # one more image would fit the tile and N / want allows it: the cap of 2048 outputs is what stops G
    ("G limited by the output cap, short last group", (1,), [((9, 1024, 16, 16), "plain")],
     lambda i: 1 < i["G"] < i["N"] // i["want"] and _dw_fits_out(i, i["G"]) and not _dw_fits_out(i, i["G"] + 1) and
     _dw_fits_tile(i, i["G"] + 1) and i["N"] % i["G"] != 0),
    ("G limited by the staged tile, a plane that is all halo", (1,), [((460, 1024, 1, 1), "plain")],
     lambda i: i["H"] == i["W"] == 1 and 1 < i["G"] < i["N"] // i["want"] and _dw_fits_tile(i, i["G"]) and
     not _dw_fits_tile(i, i["G"] + 1) and _dw_fits_out(i, i["G"] + 1)),
    ("G limited by N / want, MobileNetV2's last stage at batch 128", (1, 2), [((128, 960, 2, 2), "plain")],
     lambda i: 1 < i["G"] == i["N"] // i["want"] < i["N"] and _dw_fits_tile(i, i["G"] + 1) and
     _dw_fits_out(i, i["G"] + 1)),
    # the last band's input rows end at H, not at 2 Ho, in every image of the group
    ("stride 2, G>1, odd H", (2,), [((6, 512, 7, 8), "plain")], lambda i: i["G"] > 1 and i["H"] % 2 == 1),
    ("stride 2, G>1, even H", (2,), [((6, 512, 6, 8), "plain")], lambda i: i["G"] > 1 and i["H"] % 2 == 0),
]
DWBN_CASES = [(name, s) for name, strides, _, _ in DWBN for s in strides]
# make_inputs(shape, stride, seed): sum(shape) + stride unless a shape misses the clip coverage with it
DWBN_SEEDS = {}


def dwbn_seed(shape, stride):
    return DWBN_SEEDS.get((tuple(shape), stride), sum(shape) + stride)


def dwbn(name, stride, dtype):
    """The smallest candidate of the named dwbn branch at this stride and type: dwbn_info plus `shape` and `numel`."""
    (strides, cands, pred), = [(b[1], b[2], b[3]) for b in DWBN if b[0] == name]
    assert stride in strides, (name, stride)
    found = []
    for shape, layout in cands:
        i = dwbn_info(shape, layout, stride, dtype)
        if pred(i):
            i.update(shape=shape, numel=numel(shape))
            found.append(i)
    return _smallest("dwbn", f"{name} (stride {stride}, {dtype})", found)


# --------------------------------------------------------------------------------------------------- bnact, densebn
def walk_info(plan, m, hw, vec):
    """How the S workgroups of a channel walk their spans in steps of 256 * vec values: the longest walk, one step in
    (image, position), whether the last step of the channel is partial, and `wraps`: the steps a lane takes and goes on
    from (its next position is still its own) in which the position passes the end of a plane, so that the image
    advances by one more than step_q.  A wrap on a lane's last step changes nothing that lane reads or writes."""
    step = 256 * vec
    own = [min(m, (s + 1) * plan["span"]) - s * plan["span"] for s in range(plan["S"])]
    assert min(own) > 0 and sum(own) == m, (plan, m)
    wraps = 0
    for s in range(plan["S"]):
        end = s * plan["span"] + own[s]
        for t in range(256):
            at = s * plan["span"] + t * vec
            while at + step < end:
                wraps += at % hw + step % hw >= hw
                at += step
    return dict(M=m, HW=hw, vec=vec, steps=max(-(-v // step) for v in own), step_q=step // hw, step_r=step % hw,
                partial=m % step != 0, wraps=wraps)


def bnact_info(shape, layout, dtype):
    n, c, h, w = shape
    v = lanes(dtype)
    i = dict(ops.bnact_plan(n, c, h, w, dtype))
    i["per"] = i["span"] // (256 * v)
    width_ok = (h * w) % v == 0
    i.update(walk_info(i, n * h * w, h * w, v if width_ok and layout == "plain" else 1))
    i.update(dtype=dtype, layout=layout, width_ok=width_ok)
    return i


# (name, [(shape, layout of every tensor)], predicate on bnact_info)
BNACT = [
    ("element walk, several steps that cross planes", [((8, 3, 7, 7), "plain")],
     lambda i: i["vec"] == 1 and i["steps"] > 1 and i["step_q"] >= 1 and i["step_r"] > 0 and i["wraps"] > 0 and
     i["M"] % 256 != 0),
    # 15 images are three float32 trips; of two 16-bit trips the second then holds no lane that has wrapped: 16 images
    ("16-byte walk, several trips that cross planes, partial last trip",
     [((15, 2048, 12, 12), "plain"), ((16, 2048, 12, 12), "plain")],
     lambda i: i["vec"] > 1 and i["per"] > 1 and i["steps"] > 1 and i["step_q"] >= 1 and i["step_r"] > 0 and
     i["wraps"] > 0 and i["partial"]),
    ("16-byte walk, several trips of whole planes", [((17, 2048, 8, 8), "plain"), ((33, 2048, 8, 8), "plain")],
     lambda i: i["vec"] > 1 and i["per"] > 1 and i["steps"] > 1 and i["step_q"] >= 1 and i["step_r"] == 0),
]


def bnact(name, dtype):
    """The smallest candidate of the named bnact branch for this type: bnact_info plus `shape` and `numel`."""
    (cands, pred), = [(b[1], b[2]) for b in BNACT if b[0] == name]
    found = []
    for shape, layout in cands:
        i = bnact_info(shape, layout, dtype)
        if pred(i):
            i.update(shape=shape, numel=numel(shape))
            found.append(i)
    return _smallest("bnact", f"{name} ({dtype})", found)


def densebn_info(layout, dtype):
    """`layout` = (channels of the segments, N, H, W, index of the misaligned segment or None), the tuples of
    tests/test_gpu_densebn.py: the consumer's plan and walk, and every segment's statistics plan and walk."""
    chans, n, h, w, odd = layout
    v = lanes(dtype)
    width_ok = (h * w) % v == 0
    i = dict(ops.densebn_plan(n, chans, h, w, dtype))
    i["per"] = i["span"] // (256 * v)
    i.update(walk_info(i, n * h * w, h * w, v if width_ok and odd is None else 1))
    i["stats"] = []
    for k, ck in enumerate(chans):
        sp = dict(ops.densebn_plan(n, (ck,), h, w, dtype))
        sp.update(walk_info(sp, n * h * w, h * w, v if width_ok and odd != k else 1))
        i["stats"].append(sp)
    i.update(dtype=dtype, odd=odd, width_ok=width_ok)
    return i


# (name, [layout], predicate on densebn_info)
DENSEBN = [
    ("element walk, several steps that cross planes", [((5, 3, 3), 8, 7, 7, None)],
     lambda i: i["vec"] == 1 and not i["width_ok"] and i["steps"] > 1 and i["step_q"] >= 1 and i["step_r"] > 0 and
     i["wraps"] > 0 and all(s["steps"] > 1 and s["wraps"] > 0 for s in i["stats"])),
    ("element walk by a misaligned segment, several steps that cross planes", [((8, 4, 4), 7, 6, 8, 1)],
     lambda i: i["vec"] == 1 and i["width_ok"] and i["odd"] is not None and i["steps"] > 1 and i["step_q"] >= 1 and
     i["step_r"] > 0 and i["wraps"] > 0),
    # the statistics launch of every segment plans another S and span than the consumer of all of them; 16 images for
    # the 16-bit types, as in BNACT
    ("16-byte walk, several trips that cross planes, partial last trip, other statistics plans",
     [((1024, 512, 512), 15, 12, 12, None), ((1024, 512, 512), 16, 12, 12, None)],
     lambda i: i["vec"] > 1 and i["per"] > 1 and i["steps"] > 1 and i["step_q"] >= 1 and i["step_r"] > 0 and
     i["wraps"] > 0 and i["partial"] and all(s["S"] != i["S"] and s["span"] != i["span"] for s in i["stats"])),
    ("more than 64 splits: both halves of the fixed-order sum", [((1, 1), 65, 32, 32, None), ((1, 1), 130, 32, 32, None)],
     lambda i: i["S"] > 64),
]
DENSEBN_EVAL_AND_F16 = [DENSEBN[0][0], DENSEBN[2][0]]


def densebn(name, dtype):
    """The smallest candidate of the named densebn branch for this type: densebn_info plus `layout` and `numel`."""
    (cands, pred), = [(b[1], b[2]) for b in DENSEBN if b[0] == name]
    found = []
    for layout in cands:
        i = densebn_info(layout, dtype)
        if pred(i):
            i.update(layout=layout, numel=layout[1] * sum(layout[0]) * layout[2] * layout[3])
            found.append(i)
    return _smallest("densebn", f"{name} ({dtype})", found)
