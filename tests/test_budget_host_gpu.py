"""The update budget chosen on the device, through the C++ processors (ProgressivePhotonTracerCL.budgetOnDevice): a 10 % budget, a TF
edit, the refinement timer's evaluations until nothing is pending -- the photons of the same network with the property off, bit for
bit, batch by batch, and no host wait between the importance pass and the splat."""
import numpy as np
import pytest

from test_parity_gpu import bits
from test_host_layer_gpu import _light

pytestmark = pytest.mark.gpu

BASE = [(0.0, 1, 1, 1, 0.0), (0.45, 1, 0.5, 0.2, 0.0), (0.55, 0.6, 0.3, 0.1, 0.05), (0.8, 0.9, 0.2, 0.3, 0.4), (1.0, 0.1, 0.6, 0.7, 0.5)]
EDIT = BASE[:3] + [(0.85,) + BASE[3][1:]] + BASE[4:]
N_SIDE, PCT = 160, 10.0


@pytest.fixture(scope="module")
def hostlib(cpm, ctx):
    # ctx first: torch brings up its HIP runtime before libcpm_host.so binds one
    import importlib
    return importlib.import_module(cpm.__name__ + ".hostlayer")


def _network(hostlib, lib, cpm, on_device):
    S = cpm.synthetic
    pos, d = _light(cpm, (0.3, 0.5, -1.0))
    net = hostlib.HostNetwork(lib, S.heterogeneous_volume(64), N_SIDE, pos, d, BASE, correlated=True)
    net.set_float("tracer", "maxIncrementalPhotonsToUpdate", PCT)
    net.set_string("tracer", "importanceBranchPolicy", "always")
    if on_device:
        net.set_float("tracer", "budgetOnDevice", 1.0)
    net.evaluate(first=True)
    net.set_float("lightvolume", "incrementalRecomputationThreshold", 100.0)
    return net


def test_budget_on_device_through_the_processors(hostlib, cpm, ctx):
    S = cpm.synthetic
    lib = hostlib.load()
    off, on = _network(hostlib, lib, cpm, False), _network(hostlib, lib, cpm, True)
    budget = ctx.update_budget(on.n_photons, PCT)
    assert budget == 2560
    before = on.photons()
    for pts in (EDIT, BASE):                      # a second edit after the first has been served in full
        waits_off, waits_on = off.host_waits, on.host_waits
        for net in (off, on):
            net.set_transfer_function(pts)
            net.evaluate()
        assert on.last_decision == "importance branch (budget on device)"
        assert on.last_path == "incremental" and off.last_path in ("incremental", "full")   # (the legacy network's first add-remove needs a snapshot)
        assert on.n_recomputed == off.n_recomputed == budget
        remaining = on.remaining
        assert remaining == off.remaining > budget          # the budget binds, more than one continuation to come
        n_changed = budget + remaining
        evaluations = 1
        while True:
            assert np.array_equal(bits(on.photons()), bits(off.photons())), evaluations
            if on.remaining == 0:
                break
            for net in (off, on):
                net.refine()
            evaluations += 1
            assert on.last_decision == "importance branch continuation (budget on device)"
            assert on.last_path == "incremental"
            assert on.n_recomputed == off.n_recomputed == min(budget, remaining)
            remaining -= on.n_recomputed
            assert on.remaining == off.remaining == remaining
        assert evaluations == -(-n_changed // budget)
        # the device-resident network never blocked on a count between its importance pass and its trace; the other one did, once per edit
        assert on.host_waits == waits_on
        assert off.host_waits == waits_off + 1
        fresh = hostlib.HostNetwork(lib, S.heterogeneous_volume(64), N_SIDE, *_light(cpm, (0.3, 0.5, -1.0)), pts, correlated=False)
        fresh.evaluate(first=True)
        assert np.array_equal(bits(on.photons()), bits(fresh.photons()))
        fresh.close()
    assert (bits(on.photons()) == bits(before)).all()       # edited and reverted: the first frame's photons again
    off.close(); on.close()
