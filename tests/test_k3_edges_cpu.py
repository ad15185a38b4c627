"""tests/k3edges.py holds what it promises (CPU): the oracle's k-th largest is torch.topk's
minimum on every key set and lattice, every window case takes the route its row names and has
the counts its row states, and the oracle's sparsify takes the ``ok`` branch at the designed key."""
import numpy as np
import pytest
import torch

import k3edges as K
from oracle import dgc_oracle as O

F32, U32 = np.float32, np.uint32


def bits(x):
    return int(np.asarray(x, F32).reshape(1).view(U32)[0])


def topk_min(mag, k):
    return torch.topk(torch.from_numpy(mag), k, sorted=False)[0].min().numpy()


def same(a, b):
    return (np.isnan(a) and np.isnan(b)) or bits(a) == bits(b)


@pytest.mark.parametrize("name", list(K.key_sets()))
def test_key_set_oracle_is_topk_min(name):
    s = K.key_sets()[name]
    mag = np.abs(s.x)
    assert s.ks and all(1 <= k <= mag.size for k in s.ks)
    ks = s.ks if mag.size <= 4096 * 512 + 1 else (1, 2, mag.size)   # (torch's topk sorts: keep it quick)
    for k in ks:
        assert same(O.kth_largest(mag, k), topk_min(mag, k)), (name, k)


def test_key_sets_are_what_they_say():
    sets = K.key_sets()
    sizes = {int(n[5:]) for n in sets if n.startswith("size_")}
    assert sizes == set(K.ONE_WG_SIZES + K.MULTI_SIZES)
    for t in (0x3F800000, 0x3F7FFFFF, 0, 1, 0x7F7FFFFF, 0x7F800000):
        for tag in ("wg", "mb"):
            s = sets[f"digit_{t:08x}_{tag}"]
            got = {int(K.keys_of([O.kth_largest(np.abs(s.x), k)])[0]) for k in s.ks}
            assert t in got, (hex(t), tag)
    for p, b in (("p0", 0x3FA00000), ("p1", 0x3F800400), ("p2", 0x3F800401)):
        for tag in ("wg", "mb"):
            s = sets[f"boundary_{p}_{tag}"]
            got = {int(K.keys_of([O.kth_largest(np.abs(s.x), k)])[0]) for k in s.ks}
            assert {b, b - 1} <= got, (p, tag)
    for tag in ("wg", "mb"):
        s = sets[f"run_{tag}"]
        got = [bits(O.kth_largest(np.abs(s.x), k)) for k in s.ks]
        assert got.count(0x3E99999A) >= 3
        z = sets[f"zeros_{tag}"].x
        assert (K.keys_of(z) == 0).any() and (z.view(U32) == 0x80000000).any() and (z.view(U32) == 0).any()
        assert np.isnan(sets[f"nan_{tag}"].x).sum() == 1
    # the floor adversaries: the k-th largest per-thread maximum against the true k-th key
    for layout in ("vec", "scalar"):
        for n in (K.SMALL_N, 20003):
            s = sets[f"floor_one_thread_{layout}_{n}"]
            keys = K.keys_of(s.x)
            mx = np.array([keys[K.owner_slots(layout, t, n)].max(initial=0) for t in range(K.THREADS)])
            kth_max, kth = np.sort(mx)[::-1][19], np.sort(keys)[::-1][19]
            assert (int(kth) >> 21) - (int(kth_max) >> 21) > 8, (layout, n)   # many pass-0 bins apart
        s = sets[f"floor_one_each_{layout}"]
        keys = K.keys_of(s.x)
        per = [int((keys[K.owner_slots(layout, t, K.SMALL_N)] >= 0x44800000).sum()) for t in range(K.THREADS)]
        assert per == [1] * K.THREADS and {1023, 1024, 1025} <= set(s.ks)
        assert bits(O.kth_largest(np.abs(s.x), 1024)) == 0x44800000 and (keys >> 21).max() == 0x44800000 >> 21
    assert max(sets["floor_none_vec_700"].ks) > 700 // 4 and sets["floor_none_vec_700"].x.size < 1024
    assert max(sets["floor_none_scalar_1500"].ks) > K.THREADS


ROWS = {   # the issue's table: row -> (route, window_keys is cnt?)
    "eq_ks": ("hist", True), "eq_ks_spec0": ("hist", True), "short": ("samples", False), "at_wk": ("hist", True),
    "cap": ("hist", True), "cap+1": ("samples", False), "bin_4093": ("hist", True), "bin_4094": ("window_wg", True),
    "bin_4096": ("hist", True), "bin_4097": ("window_wg", True), "ties_first": ("hist", True),
    "ties_mid": ("hist", True), "ties_last": ("hist", True), "inf_few": ("hist", True),
    "inf_many": ("window_wg", True), "nan": ("hist", True), "span_0": ("window_wg", True),
    "span_4095": ("window_wg", True), "span_4096": ("window_wg", True), "span_2p24m1": ("window_wg", True),
    "span_2p24": ("window_wg", True), "tail": ("samples", False), "edge_S_32768": ("small", False),
    "edge_S_32769": ("hist", True), "big_hist": ("hist", True), "big_wg": ("window_wg", True),
    "big_passes": ("window_passes", True), "big_passes_bin": ("window_passes", True),
}


def test_every_row_is_present():
    assert set(K.window_cases()) == set(ROWS)
    capw, capb = K.win_cap_of(K.N_W // K.STRIDE), K.win_cap_of(K.N_WBIG // K.STRIDE)
    assert capw == (35000 + 1) // 16 + 4096 and 4097 < capw < K.WIN_MAX      # room for a 4097-key bin
    assert capb == (1_000_000 + 1) // 16 + 4096 and capb > K.WIN_MAX + 1     # room for 65537 keys


@pytest.mark.parametrize("name", list(ROWS))
def test_window_case_is_what_it_says(name):
    c = K.window_cases()[name]
    want_route, windowed = ROWS[name]
    e = c.expect
    keys, wk = K.lattice_keys(c), K.window_key(c)
    mag = np.abs(c.grad)
    lat = mag[c.start::c.stride]
    assert lat.size == e["samples"] and e["S"] == c.N // c.stride and e["samples"] <= e["S"] + 1
    # the oracle's threshold is topk's minimum, and the designed key
    t0 = O.kth_largest(lat, c.ks)
    assert same(t0, topk_min(lat, c.ks)), name
    assert same(t0, K.f32_of([c.t0_key])[0]), name
    # the route and the record's window_keys
    win = keys[keys >= wk]
    assert win.size == e["cnt"], name
    assert K.route(c) == (want_route, e["cnt"] if windowed else 0), (name, K.route(c))
    assert c.route == want_route and c.window_keys == (e["cnt"] if windowed else 0), name
    # the counts the row states
    cap = e["win_cap"]
    exact = {"eq_ks": c.ks, "eq_ks_spec0": c.ks, "at_wk": c.ks, "short": c.ks - 1, "cap": cap, "cap+1": cap + 1,
             "big_wg": K.WIN_MAX, "big_passes": K.WIN_MAX + 1, "big_passes_bin": K.WIN_MAX + 1}
    if name in exact:
        assert e["cnt"] == exact[name], name
    if name == "big_hist":
        assert K.WIN_MAX < e["cnt"] <= cap
    if name == "short":
        assert c.t0_key == wk - 1
    if name == "at_wk":
        assert c.t0_key == wk
    if name == "eq_ks":
        assert c.t0_key == int(win.min())
    if name == "eq_ks_spec0":
        assert np.isinf(c.spec2) and np.isfinite(c.spec0)
    else:
        assert np.isinf(c.spec0) and np.isfinite(c.spec2)
    if name == "bin_4093":
        assert c.t0_key == wk + 4094 * 1024 - 1
    if name == "bin_4094":
        assert c.t0_key == wk + 4094 * 1024
    if name.startswith("inf"):
        n_inf = int((keys == K.INF_KEY).sum())
        assert (n_inf < c.ks) == (name == "inf_few") and (c.t0_key == K.INF_KEY) == (name == "inf_many")
    if name == "nan":
        assert int((keys > K.INF_KEY).sum()) == 1 and np.isnan(t0)
    if "kth_bin" in e:
        assert min((c.t0_key - wk) >> K.WIN_SHIFT, K.WIN_BINS - 2) == e["kth_bin"], name
    if "kth_bin_count" in e:
        b = np.minimum((win - wk) >> K.WIN_SHIFT, K.WIN_BINS - 2)
        assert int((b == e["kth_bin"]).sum()) == e["kth_bin_count"], name
        if name.startswith("bin_409"):   # distinct sub-bins: every one of the 1024 is used
            assert np.unique(win[b == e["kth_bin"]]).size == K.BIN
    if "ties_at_t0" in e:
        assert int((keys == c.t0_key).sum()) == e["ties_at_t0"], name
        above = int((keys > c.t0_key).sum())
        where = {"ties_first": 1, "ties_mid": e["ties_at_t0"] // 2, "ties_last": e["ties_at_t0"]}
        if name in where:
            assert c.ks == above + where[name]
    if "span" in e:
        assert int(win.max() - win.min()) == e["span"], name
        if "passes" in e:
            assert K.window_passes_of(e["span"]) == e["passes"], name
    if "blocks" in e:
        assert -(-e["cnt"] // 4096) == e["blocks"]
    if name.startswith("edge_S"):
        assert e["S"] + 1 == int(name[-5:]) and (name != "edge_S_32768" or e["samples"] == K.SMALL_N)
    if name == "tail":
        assert c.N == K.N_W + 1 and c.N % 4
    # off the lattice: non-zero bulk far below the window key, so the count at t0 is num_selects
    off = np.ones(c.N, bool)
    off[c.start::c.stride] = False
    assert mag[off].min() > 0 and mag[off].max() < K.f32_of([wk])[0] / 16, name
    assert 0 < int((c.grad < 0).sum()) < c.N
    # the oracle's run: the ok branch at the designed key, nothing lowered
    attrs = (c.N, c.k, e["S"], c.ks, c.stride)
    v, i, info = O.sparsify(c.grad.copy(), attrs, c.start)
    assert same(info["thresholds"][0], K.f32_of([c.t0_key])[0]), name
    if name == "nan":
        assert info["branch"] == "exhausted" and i.size == 0
    else:
        assert info["branch"] == "ok" and len(info["counts"]) == 1, (name, info["branch"], info["counts"])
        assert int(info["counts"][0]) == e["count_at_t0"] == c.k == i.size, name
    if name not in ("span_0", "nan") and not name.startswith("span_"):
        assert c.k == (K.K_WBIG if c.N == K.N_WBIG else K.K_W), name   # one workspace layout per size


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("kind", list(K.ENGINE_ROWS))
def test_engine_row_is_what_it_says(kind, dtype):
    """The rows of the bucket and batch tests, on the smallest windowed tensor of the
    reference's own attributes: route, counts, representable values, the oracle's branch."""
    N = K.smallest_windowed_numel()
    attrs = O.attributes(N, 0.001)
    assert attrs[2] + 1 > K.SMALL_N and O.attributes(N - 1, 0.001)[2] + 1 <= K.SMALL_N
    wk = K.WK if dtype != "float32" else int(K.keys_of([F32(0.9) * F32(0.3085)])[0])
    c = K.engine_row(kind, attrs, 5, wk, dtype, seed=3)
    e = c.expect
    assert (c.N, c.k, e["S"], c.ks, c.stride) == attrs
    if dtype != "float32":
        assert np.array_equal(O.round16(c.grad, dtype).view(U32), c.grad.view(U32))   # representable
    keys = K.lattice_keys(c)
    win = keys[keys >= wk]
    assert win.size == e["cnt"] and int((keys == wk - K.KEY_STEP[dtype]).sum()) == 1
    assert K.route(c, padded=True) == (K.ENGINE_ROWS[kind], 0 if kind == "cap+1" else e["cnt"]), K.route(c, True)
    assert c.window_keys == K.route(c, padded=True)[1]
    if kind == "cap+1":
        assert e["cnt"] == e["win_cap"] + 1
    if kind == "eq_ks":
        assert e["cnt"] == c.ks and c.t0_key == int(win.min())
    if "kth_bin" in e:
        assert min((c.t0_key - wk) >> K.WIN_SHIFT, K.WIN_BINS - 2) == e["kth_bin"]
    if "kth_bin_count" in e:
        b = np.minimum((win - wk) >> K.WIN_SHIFT, K.WIN_BINS - 2)
        assert int((b == e["kth_bin"]).sum()) == e["kth_bin_count"] == K.WIN_BIN_CAP + 1
        assert int((keys == c.t0_key).sum()) == e["ties_at_t0"]
    mag = np.abs(c.grad)
    assert same(O.kth_largest(mag[c.start::c.stride], c.ks), K.f32_of([c.t0_key])[0])
    v, i, info = O.sparsify(c.grad.copy(), attrs, c.start)
    assert same(info["thresholds"][0], K.f32_of([c.t0_key])[0])
    if e["count_at_t0"] == c.k:
        assert info["branch"] == "ok" and len(info["counts"]) == 1
    else:   # a 16-bit bin of 4097 equal samples holds more than num_selects: first k or resample
        assert kind == "bin_4097" and dtype != "float32" and info["branch"] in ("trunc", "resample")
