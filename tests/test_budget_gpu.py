"""The budgeted correlated update on the device (cpm_selection_select_pending, cpm_selection_finish_budget, cpm_selection_counts):
the `budget` most important changed photons -- smallest key, ties by index -- as an ascending list, chosen without a sort and without
a host read.  The expected selection is numpy's (lexsort by (key, index), the first m, sorted by index) and, where stated, today's
chain (cpm_select_recompute + the first m + cpm_sort_keys).  160^2 photons and a 32^3 light volume, as the other correlated tests."""
import numpy as np
import pytest

from test_parity_gpu import _t, _n, bits

pytestmark = pytest.mark.gpu
UNCHANGED = 2147483647
N_SIDE = 160
N = N_SIDE * N_SIDE


def want_selection(keys, spans, budget):
    """(list, m, |C|) by the contract: C = photons of the spans with key < 0x7fffffff, the first m = min(|C|, budget) by (key, index)."""
    index = np.concatenate([np.arange(o, o + c) for o, c in spans]).astype(np.int64) if spans else np.zeros(0, np.int64)
    index = index[keys[index] < UNCHANGED]
    key = keys[index]
    order = index[np.lexsort((index, key))]
    m = min(order.size, budget)
    return np.sort(order[:m]).astype(np.uint32), m, order.size


def device_selection(ctx, sel, keys_d, idx_d, spans, budget):
    sel.begin()
    for off, cnt in spans:
        sel.select_pending(keys_d, off, cnt)
    sel.finish(idx_d, budget=budget, importances=keys_d)
    m, c = sel.counts()
    assert sel.count() == m
    return _n(idx_d, np.uint32)[:m].copy(), m, c


def _key_cases():
    rng = np.random.default_rng(11)
    cases = {}
    k = rng.integers(0, UNCHANGED, N, dtype=np.uint32)
    k[rng.random(N) < 0.3] = UNCHANGED
    cases["random31"] = k
    k = rng.choice(np.array([5, 1 << 20, (1 << 20) + 1, UNCHANGED - 1], np.uint32), N)
    k[rng.random(N) < 0.5] = UNCHANGED
    cases["four_values"] = k
    k = np.full(N, UNCHANGED, np.uint32)
    k[::3] = UNCHANGED - 100
    cases["all_equal"] = k
    k = rng.integers(0, 1 << 12, N, dtype=np.uint32) << 10     # keys that agree in their low digit: the cut falls in the middle one
    k[rng.random(N) < 0.2] = UNCHANGED
    cases["low_digit_zero"] = k
    return cases


@pytest.mark.parametrize("case", ["random31", "four_values", "all_equal", "low_digit_zero"])
def test_selection_by_rank_equals_numpy(ctx, case):
    """Keys written by the test; budgets around |C| and the tile sizes; one light and two; twice the same call."""
    keys = _key_cases()[case]
    n_c = int((keys < UNCHANGED).sum())
    keys_d = _t(ctx, keys)
    idx_d = ctx.torch.full((N,), -1, dtype=ctx.torch.int32, device=ctx.device)
    sel = ctx.selection_create(N)
    one, two = [(0, N)], [(0, 13001), (13001, N - 13001)]
    for spans in (one, two):
        for budget in (0, 1, 2, 255, 256, 257, 1280, n_c // 2, n_c - 1, n_c, n_c + 1, N, UNCHANGED):
            want, wm, wc = want_selection(keys, spans, budget)
            got, m, c = device_selection(ctx, sel, keys_d, idx_d, spans, budget)
            assert (m, c) == (wm, wc) and wc == n_c, (case, budget)
            assert np.array_equal(got, want), (case, budget)
            again, m2, c2 = device_selection(ctx, sel, keys_d, idx_d, spans, budget)
            assert (m2, c2) == (m, c) and np.array_equal(again, got)
    assert np.array_equal(_n(keys_d, np.uint32), keys)          # no key was written
    sel.close()


def test_selection_edge_cases(ctx):
    """|C| = 0, |C| < B, |C| == B, n not a multiple of the tile size, a sub-range of the photons, an empty selection; a budget that covers
    everything gives cpm_selection_finish's list and count, bit for bit."""
    torch = ctx.torch
    rng = np.random.default_rng(5)
    n = N + 37
    keys = rng.integers(0, UNCHANGED, n, dtype=np.uint32)
    keys[rng.random(n) < 0.6] = UNCHANGED
    idx_d = torch.full((n,), -1, dtype=torch.int32, device=ctx.device)
    sel = ctx.selection_create(n)
    none_d = _t(ctx, np.full(n, UNCHANGED, np.uint32))
    got, m, c = device_selection(ctx, sel, none_d, idx_d, [(0, n)], 100)
    assert (m, c) == (0, 0)
    keys_d = _t(ctx, keys)
    n_c = int((keys < UNCHANGED).sum())
    for spans in ([(0, n)], [(5, n - 5)], [(0, 1000), (1000, 1)], [(300, 77), (377, n - 377)]):
        _, _, wc = want_selection(keys, spans, 0)
        for budget in (wc + 10, wc, max(wc - 1, 0), wc // 3):
            want, wm, _ = want_selection(keys, spans, budget)
            got, m, c = device_selection(ctx, sel, keys_d, idx_d, spans, budget)
            assert (m, c) == (wm, wc) and np.array_equal(got, want), (spans, budget)
    # budget >= |C| == the plain finish on the same selection state
    ref_d = torch.full((n,), -1, dtype=torch.int32, device=ctx.device)
    sel.begin()
    sel.select_pending(keys_d, 0, n)
    sel.finish(ref_d)
    cnt = sel.count()
    assert sel.counts() == (cnt, cnt) and cnt == n_c
    for budget in (n_c, n, UNCHANGED):
        idx_d.fill_(-1)
        got, m, c = device_selection(ctx, sel, keys_d, idx_d, [(0, n)], budget)
        assert (m, c) == (cnt, cnt)
        assert np.array_equal(_n(idx_d, np.uint32), _n(ref_d, np.uint32))      # the unwritten rest included
    # nothing selected at all
    sel.begin()
    sel.finish(idx_d, budget=10, importances=keys_d)
    assert sel.counts() == (0, 0)
    sel.close()


def test_argument_errors(ctx, cpm):
    """Null selection / keys / list, negative budget, finish without begin, finish twice: CPM_ERR_INVALID_ARGUMENT, and the selection
    still works afterwards."""
    B = cpm.binding
    keys = np.full(1000, UNCHANGED, np.uint32)
    keys[::7] = 3
    keys_d = _t(ctx, keys)
    idx_d = ctx.torch.zeros(1000, dtype=ctx.torch.int32, device=ctx.device)
    lib, h = ctx.lib, ctx.h
    sel = ctx.selection_create(1000)
    assert lib.cpm_selection_finish_budget(h, sel.h, ctx._ptr(keys_d), 5, ctx._ptr(idx_d), ctx._stream()) == -1    # no begin yet
    sel.begin()
    assert lib.cpm_selection_select_pending(h, None, ctx._ptr(keys_d), 0, 1000, ctx._stream()) == -1
    assert lib.cpm_selection_select_pending(h, sel.h, None, 0, 1000, ctx._stream()) == -1
    assert lib.cpm_selection_select_pending(h, sel.h, ctx._ptr(keys_d), -1, 1000, ctx._stream()) == -1
    assert lib.cpm_selection_select_pending(h, sel.h, ctx._ptr(keys_d), 0, 1001, ctx._stream()) == -1              # beyond max_photons
    sel.select_pending(keys_d, 0, 1000)
    assert lib.cpm_selection_finish_budget(h, None, ctx._ptr(keys_d), 5, ctx._ptr(idx_d), ctx._stream()) == -1
    assert lib.cpm_selection_finish_budget(h, sel.h, None, 5, ctx._ptr(idx_d), ctx._stream()) == -1
    assert lib.cpm_selection_finish_budget(h, sel.h, ctx._ptr(keys_d), 5, None, ctx._stream()) == -1
    assert lib.cpm_selection_finish_budget(h, sel.h, ctx._ptr(keys_d), -1, ctx._ptr(idx_d), ctx._stream()) == -1
    sel.finish(idx_d, budget=5, importances=keys_d)                                                                 # ... and still works
    assert sel.counts() == (5, 143)
    assert np.array_equal(_n(idx_d, np.uint32)[:5], np.arange(0, 35, 7))
    with pytest.raises(B.CpmError):
        sel.finish(idx_d, budget=5, importances=keys_d)                                                             # twice
    assert lib.cpm_selection_counts(h, sel.h, None, None) == -1
    sel.close()


@pytest.mark.parametrize("case", ["random31", "four_values", "all_equal"])
def test_selection_equals_todays_chain(ctx, case):
    """The same keys through cpm_select_recompute (stable 31-bit sort of all keys), its first m entries, cpm_sort_keys: the list the
    legacy budgeted path traces."""
    torch = ctx.torch
    keys = _key_cases()[case]
    n_c = int((keys < UNCHANGED).sum())
    sel = ctx.selection_create(N)
    keys_d = _t(ctx, keys)
    idx_d = torch.full((N,), -1, dtype=torch.int32, device=ctx.device)
    for budget in (1, 1280, 2560, n_c - 1, n_c + 5):
        sorted_keys = _t(ctx, keys)
        ranked = torch.zeros(N, dtype=torch.int32, device=ctx.device)
        cnt = torch.zeros(1, dtype=torch.int32, device=ctx.device)
        ctx.select_recompute(sorted_keys, ranked, cnt)
        m = min(int(cnt.item()), budget)
        batch = ranked[:m].contiguous()
        ctx.sort_keys(batch, 0)
        got, gm, gc = device_selection(ctx, sel, keys_d, idx_d, [(0, N)], budget)
        assert gm == m and gc == int(cnt.item()) == n_c
        assert np.array_equal(got, _n(batch, np.uint32))
    sel.close()


# ---- through CorrelatedPhotonMapper ----------------------------------------------------------------------------------------------

BASE = [(0.0, 1, 1, 1, 0.0), (0.45, 1, 0.5, 0.2, 0.0), (0.55, 0.6, 0.3, 0.1, 0.05), (0.8, 0.9, 0.2, 0.3, 0.4), (1.0, 0.1, 0.6, 0.7, 0.5)]
EDIT = BASE[:3] + [(0.85,) + BASE[3][1:]] + BASE[4:]
EDIT2 = BASE[:2] + [(0.6,) + BASE[2][1:]] + [(0.85,) + BASE[3][1:]] + BASE[4:]
PCT = 5.0


def _mapper(ctx, cpm, vol_np, tfp, device_budget, pct=PCT, **kw):
    S, P = cpm.synthetic, cpm.pipeline
    cm = P.CorrelatedPhotonMapper(ctx, vol_np, S.tf_from_points(tfp), N_SIDE, (32, 32, 32), max_incremental_percent=pct,
                                  light_travel_direction=(0.3, 0.5, -1.0), tf_points=tfp, incremental_threshold_percent=100.0,
                                  device_budget=device_budget, **kw)
    cm.full_frame()
    return cm


def _pass_amounts(ctx, cm):
    """What the importance pass would subtract from every photon's key now: the pass on a freshly reset key buffer."""
    fresh = ctx.torch.empty(cm.n, dtype=ctx.torch.int32, device=ctx.device)
    ctx.reset_importance(fresh, 0, cm.n)
    ctx.photon_importance(cm.importance_grid, cm.brick_dims, (float(cm.region),) * 3, list(cm.vol.desc.texture_to_index), cm.photons, 0,
                          cm.light_samples, cm.isect, cm.n, cm.I, cm.n, fresh, fix_exit_point=cm.fix_exit_point)
    return (np.uint32(UNCHANGED) - _n(fresh, np.uint32)).astype(np.uint32)


def _legacy_batch(cm, n):
    """The photons the legacy mapper traced in its last evaluation, ascending (its index buffer is in ranked order)."""
    return np.sort(_n(cm.indices, np.uint32)[cm.remaining_offset - n: cm.remaining_offset])


def test_one_budgeted_evaluation_equals_the_legacy_chain(ctx, cpm):
    """A TF edit that changes more photons than a 5 % budget: photons, RNG states and the traced list of device_budget=True equal the
    legacy mapper's bit for bit; the keys of the traced photons are reset and every other key is the pre-selection key at the photon's
    own index; the light volume within the atomic splat's tolerance of the legacy add-remove (rtol 1e-3, atol 2e-5 max)."""
    S = cpm.synthetic
    vol_np = S.heterogeneous_volume(64)
    leg, dev = _mapper(ctx, cpm, vol_np, BASE, False), _mapper(ctx, cpm, vol_np, BASE, True)
    budget = ctx.update_budget(dev.n, PCT)
    assert budget == int(np.float32(PCT) / np.float32(100) * np.float32(dev.n)) == 1280
    leg.set_transfer_function(EDIT)
    dev.set_transfer_function(EDIT)
    pre = np.uint32(UNCHANGED) - _pass_amounts(ctx, dev)           # the keys after the importance pass, before the selection
    n_leg = leg.correlated_update()
    n_dev = dev.correlated_update()
    assert dev.n_changed_last > budget                              # the budget binds: not a vacuous pass
    assert n_dev == n_leg == budget and dev.remaining == leg.remaining == dev.n_changed_last - budget
    assert dev.last_path == leg.last_path == "incremental" and dev.n_recomputed == budget
    traced = _n(dev.indices, np.uint32)[:n_dev]
    assert np.array_equal(traced, _legacy_batch(leg, n_leg))
    want, wm, wc = want_selection(pre, [(0, dev.n)], budget)
    assert wc == dev.n_changed_last and np.array_equal(traced, want)
    assert np.array_equal(bits(_n(dev.photons)), bits(_n(leg.photons)))
    assert np.array_equal(_n(dev.rng, np.uint32), _n(leg.rng, np.uint32))
    keys = _n(dev.importance, np.uint32)
    assert (keys[traced] == UNCHANGED).all()
    rest = np.ones(dev.n, bool)
    rest[traced] = False
    assert np.array_equal(keys[rest], pre[rest])
    lv_leg, lv_dev = _n(leg.light_volume), _n(dev.light_volume)
    np.testing.assert_allclose(lv_dev, lv_leg, rtol=1e-3, atol=2e-5 * float(lv_leg.max()))


def test_continuation_walks_the_stable_sort(ctx, cpm):
    """continue_update until nothing is pending: every evaluation traces what the legacy mapper's traces, ceil(|C| / B) evaluations,
    then the photons are those of a full re-trace with the new TF and every key is back at 0x7fffffff."""
    S, P = cpm.synthetic, cpm.pipeline
    vol_np = S.heterogeneous_volume(64)
    leg, dev = _mapper(ctx, cpm, vol_np, BASE, False), _mapper(ctx, cpm, vol_np, BASE, True)
    budget = ctx.update_budget(dev.n, PCT)
    leg.set_transfer_function(EDIT)
    dev.set_transfer_function(EDIT)
    n_leg, n_dev = leg.correlated_update(), dev.correlated_update()
    n_changed = dev.n_changed_last
    assert n_changed > budget
    evaluations = 1
    while True:
        assert n_dev == n_leg and dev.remaining == leg.remaining
        assert np.array_equal(_n(dev.indices, np.uint32)[:n_dev], _legacy_batch(leg, n_leg)), evaluations
        if dev.remaining == 0:
            break
        n_leg, n_dev = leg.continue_update(), dev.continue_update()
        evaluations += 1
        assert evaluations <= dev.n
    assert evaluations == -(-n_changed // budget)
    assert dev.continue_update() == 0
    full = P.PhotonFrame(ctx, vol_np, S.tf_from_points(EDIT), N_SIDE, (32, 32, 32), light_travel_direction=(0.3, 0.5, -1.0))
    full.trace()
    assert np.array_equal(bits(_n(dev.photons)), bits(_n(full.photons)))
    assert (_n(dev.importance, np.uint32) == UNCHANGED).all()


def test_second_edit_while_a_continuation_is_pending(ctx, cpm):
    """After a budgeted evaluation a second edit's importance pass subtracts from the keys at the photons' own indices: every still
    pending photon's key is 0x7fffffff - (first pass's amount) - (second pass's amount), plain u32 arithmetic."""
    S = cpm.synthetic
    vol_np = S.heterogeneous_volume(64)
    dev = _mapper(ctx, cpm, vol_np, BASE, True)
    budget = ctx.update_budget(dev.n, PCT)
    dev.set_transfer_function(EDIT)
    a1 = _pass_amounts(ctx, dev)
    n1 = dev.correlated_update()
    s1 = _n(dev.indices, np.uint32)[:n1].copy()
    assert dev.remaining > 0 and n1 == budget
    model = np.uint32(UNCHANGED) - a1
    model[s1] = UNCHANGED
    assert np.array_equal(_n(dev.importance, np.uint32), model)
    dev.set_transfer_function(EDIT2)
    a2 = _pass_amounts(ctx, dev)                                    # (on the photons as they are now: s1 re-traced)
    assert (a2 > 0).any()
    assert (model.astype(np.int64) - a2.astype(np.int64) >= 0).all()   # no key wraps
    model = model - a2
    want, wm, wc = want_selection(model, [(0, dev.n)], budget)
    n2 = dev.correlated_update()
    s2 = _n(dev.indices, np.uint32)[:n2]
    assert wc > budget and n2 == wm == budget and dev.n_changed_last == wc
    assert np.array_equal(s2, want)
    keys = _n(dev.importance, np.uint32)
    pending = model < UNCHANGED
    pending[s2] = False
    assert pending.sum() == dev.remaining > 0
    assert np.array_equal(keys[pending], model[pending])
    assert (keys[~pending] == UNCHANGED).all()
    # ... and the continuation drains exactly them, most important first
    while dev.remaining > 0:
        model[s2] = UNCHANGED
        want, wm, _ = want_selection(model, [(0, dev.n)], budget)
        n2 = dev.continue_update()
        s2 = _n(dev.indices, np.uint32)[:n2].copy()
        assert n2 == wm and np.array_equal(s2, want)
    assert (_n(dev.importance, np.uint32) == UNCHANGED).all()


def test_equal_importance_detector_with_a_budget(ctx, cpm):
    """Every fourth photon changed, all keys equal: the index rule is the whole selection; evaluation + continuation."""
    S, P = cpm.synthetic, cpm.pipeline
    vol_np = S.heterogeneous_volume(64)
    with pytest.raises(ValueError):
        P.CorrelatedPhotonMapper(ctx, vol_np, S.tf_from_points(BASE), N_SIDE, (32, 32, 32), detector="equal")   # only the budgeted device path serves it
    dev = _mapper(ctx, cpm, vol_np, BASE, True, detector="equal", equal_percentage=25)
    before = _n(dev.photons).copy()
    budget = ctx.update_budget(dev.n, PCT)
    dev.set_transfer_function(EDIT)
    changed = np.arange(0, dev.n, 4, dtype=np.uint32)
    n = dev.correlated_update()
    evaluations = 1
    assert dev.n_changed_last == changed.size > budget
    while True:
        lo = (evaluations - 1) * budget
        assert np.array_equal(_n(dev.indices, np.uint32)[:n], changed[lo: lo + budget]), evaluations
        if dev.remaining == 0:
            break
        n = dev.continue_update()
        evaluations += 1
    assert evaluations == -(-changed.size // budget)
    full = P.PhotonFrame(ctx, vol_np, S.tf_from_points(EDIT), N_SIDE, (32, 32, 32), light_travel_direction=(0.3, 0.5, -1.0))
    full.trace()
    after = _n(dev.photons)
    assert np.array_equal(bits(after[changed]), bits(_n(full.photons)[changed]))
    rest = np.ones(dev.n, bool)
    rest[changed] = False
    assert np.array_equal(bits(after[rest]), bits(before[rest]))
    assert (_n(dev.importance, np.uint32) == UNCHANGED).all()


def test_time_step_with_a_budget(ctx, cpm):
    """set_volume, a budgeted evaluation and its continuation: evaluation by evaluation the legacy mapper's photons."""
    S = cpm.synthetic
    tfp = [(0.0, 1, 1, 1, 0.0), (0.55, 1, 0.5, 0.2, 0.0), (0.7, 0.6, 0.3, 0.1, 0.3), (1.0, 0.1, 0.6, 0.7, 0.6)]
    vols = [S.heterogeneous_volume(64, S.sequence_blob_center(t * 10, 32)) for t in range(2)]
    leg, dev = _mapper(ctx, cpm, vols[0], tfp, False), _mapper(ctx, cpm, vols[0], tfp, True)
    budget = ctx.update_budget(dev.n, PCT)
    leg.set_volume(vols[1])
    dev.set_volume(vols[1])
    n_leg, n_dev = leg.correlated_update(), dev.correlated_update()
    n_changed = dev.n_changed_last
    assert n_changed > budget
    evaluations = 1
    while True:
        assert n_dev == n_leg and dev.remaining == leg.remaining
        assert np.array_equal(_n(dev.indices, np.uint32)[:n_dev], _legacy_batch(leg, n_leg)), evaluations
        assert np.array_equal(bits(_n(dev.photons)), bits(_n(leg.photons))), evaluations
        if dev.remaining == 0:
            break
        n_leg, n_dev = leg.continue_update(), dev.continue_update()
        evaluations += 1
    assert evaluations == -(-n_changed // budget)
    assert (_n(dev.importance, np.uint32) == UNCHANGED).all()
