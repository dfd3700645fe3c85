"""The XCD-aware block order of the filter's grouped tile products (`tile_map_build` in csrc/host.h) through the host-only
`tadmm_tile_map`: no device is needed.  Position i of a map is expected on XCD slot i % 8; the model charges a slot every
distinct (problem, 32- or 64-row panel of A) and (problem, panel of B) among its tiles once."""
import pytest

NX = 8
LANE0_480 = [(128, 256)] * 6 + [(160, 480)] * 3       # (r', Npad): six layer3 and three layer4 conv2 blocks of ResNet-50
LANE0_512 = [(128, 256)] * 6 + [(160, 512)] * 3

# name -> (blocks (r', Npad), tile_m, tile_n): the products Y[r'][Npad] * G[Npad][Npad]^T of one level
POPULATIONS = {
    "six_tiles": ([(64, 96)], 32, 32),
    "odd_tiles_n": ([(96, 160)], 32, 32),
    "one_480": ([(160, 480)], 32, 32),
    "lane0_480_32x32": (LANE0_480, 32, 32),
    "lane0_512_32x32": (LANE0_512, 32, 32),
    "lane0_480_64x32": (LANE0_480, 64, 32),
    "lane0_512_64x32": (LANE0_512, 64, 32),
    "four_256x512_64x32": ([(256, 512)] * 4, 64, 32),
    "tiny_and_large": ([(32, 32), (256, 512)], 32, 32),
}


def _probs(name):
    blocks, tm, tn = POPULATIONS[name]
    return [(rp, n, n, tm, tn) for rp, n in blocks]


def _grid(p):
    M, N, _, tm, tn = p
    return -(-M // tm), -(-N // tn)


def _plain(probs):
    return [(i, b) for i, p in enumerate(probs) for b in range(_grid(p)[0] * _grid(p)[1])]


def _model_bytes(m, probs):
    """The cost function of the issue, recomputed here: the library's figure must agree with it."""
    seen = set()
    total = 0
    for pos, (i, b) in enumerate(m):
        M, N, K, tm, tn = probs[i]
        cols = _grid(probs[i])[1]
        for key, rows in ((("a", b // cols), tm), (("b", b % cols), tn)):
            if (pos % NX, i, key) not in seen:
                seen.add((pos % NX, i, key))
                total += rows * K * 8
    return total


@pytest.fixture(autouse=True)
def _default_order(monkeypatch):
    for name in ("TADMM_XCD_MAP", "TADMM_TILE_MAP", "TADMM_TILE_MAP_LONGEST"):
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def ops():
    from tadmm import ops
    return ops


@pytest.mark.parametrize("name", sorted(POPULATIONS))
def test_permutation_balance_spread_and_cost(ops, name):
    probs = _probs(name)
    m, cost, cost_plain = ops.tile_map(probs)
    plain = _plain(probs)
    assert sorted(m) == plain and len(m) == len(plain), "not a permutation of the plain map"
    assert cost == _model_bytes(m, probs) and cost_plain == _model_bytes(plain, probs)
    queues = [m[x::NX] for x in range(NX)]
    assert max(map(len, queues)) - min(map(len, queues)) <= 1
    for i, p in enumerate(probs):
        tiles = _grid(p)[0] * _grid(p)[1]
        per_slot = [sum(1 for e in q if e[0] == i) for q in queues]
        if tiles >= NX:
            assert min(per_slot) >= 1, "problem %d is missing on a slot: %s" % (i, per_slot)
        assert max(per_slot) - min(per_slot) <= 1, "problem %d is not spread evenly: %s" % (i, per_slot)
    # the tiles of a slot carry nearly equal reduction length: no queue is more than one longest tile from the mean
    load = [sum(probs[i][2] for i, _ in q) for q in queues]
    assert max(load) - min(load) <= len(probs) * max(p[2] for p in probs)
    print("%s: %d blocks, %.1f MB plain, %.1f MB mapped (%.3f)" % (name, len(m), cost_plain / 1e6, cost / 1e6, cost / cost_plain))
    assert cost <= cost_plain


def test_lane0_480_level_fetches_at_most_065_of_the_plain_map(ops):
    _, cost, cost_plain = ops.tile_map(_probs("lane0_480_32x32"))
    print("lane 0, N = 480, 32 x 32: %.1f MB -> %.1f MB, ratio %.3f" % (cost_plain / 1e6, cost / 1e6, cost / cost_plain))
    assert abs(cost_plain / 1e6 - 58.1) < 0.1          # the figure of the model this order was designed on
    assert cost <= 0.65 * cost_plain


@pytest.mark.parametrize("name", ["lane0_480_32x32", "lane0_512_64x32", "tiny_and_large"])
def test_a_panel_of_g_keeps_its_slots_from_map_to_map(ops, name):
    probs = _probs(name)

    def owners(m):
        own = {}
        for pos, (i, b) in enumerate(m):
            own.setdefault((i, b % _grid(probs[i])[1]), set()).add(pos % NX)
        return own

    first, second = ops.tile_map(probs)[0], ops.tile_map(list(probs))[0]
    assert first == second
    assert owners(first) == owners(second)


def test_whole_columns_give_a_panel_of_g_at_most_two_neighbouring_slots(ops, monkeypatch):
    monkeypatch.setenv("TADMM_TILE_MAP", "2")
    probs = _probs("lane0_480_32x32")
    m = ops.tile_map(probs)[0]
    assert sorted(m) == _plain(probs)
    own = {}
    for pos, (i, b) in enumerate(m):
        own.setdefault((i, b % _grid(probs[i])[1]), set()).add(pos % NX)
    for key, slots in own.items():
        assert len(slots) <= 2 and max(slots) - min(slots) <= 1, (key, slots)


def test_longest_reductions_lead_every_slot_queue(ops, monkeypatch):
    probs = _probs("lane0_480_32x32")
    m = ops.tile_map(probs)[0]
    for x in range(NX):
        ks = [probs[i][2] for i, _ in m[x::NX]]
        assert ks == sorted(ks, reverse=True), (x, ks)
    monkeypatch.setenv("TADMM_TILE_MAP_LONGEST", "0")
    m = ops.tile_map(probs)[0]
    assert sorted(m) == _plain(probs)
    for x in range(NX):
        order = [i for i, _ in m[x::NX]]
        assert order == sorted(order), (x, order)


@pytest.mark.parametrize("env", [{"TADMM_XCD_MAP": "0"}, {"TADMM_TILE_MAP": "0"}])
def test_plain_order_on_request(ops, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    probs = _probs("lane0_480_32x32")
    m, cost, cost_plain = ops.tile_map(probs)
    assert m == _plain(probs) and cost == cost_plain


def test_refuses_empty_and_non_positive_populations(ops):
    from tadmm import _cabi
    lib = _cabi.load()
    assert lib.tadmm_tile_map(0, None, None, 0, None) == -1
    for bad in [(0, 32, 32, 32, 32), (32, 32, 32, 0, 32), (32, -32, 32, 32, 32)]:
        with pytest.raises(ValueError):
            ops.tile_map([bad])
    arr = (_cabi.TileMapProb * 1)(_cabi.TileMapProb(64, 96, 96, 32, 32))
    assert lib.tadmm_tile_map(1, arr, None, 0, None) == 6
    import ctypes as C
    out = (C.c_int32 * 12)()
    assert lib.tadmm_tile_map(1, arr, out, 5, None) < 0            # capacity below the block count
    assert lib.tadmm_tile_map(1, arr, out, 6, None) == 6
