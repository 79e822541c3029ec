"""KLD-adaptive particle counts on the GPU (include/visfs_mcl_kld.h on a device filter: k_mcl_weight, k_mcl_sums and k_mcl_finish on
the n active particles, then k_mcl_kld_resample) against the one-core host twin, byte for byte in the particles (the first n), Q,
the ancestors, every field of both results and the limit table, on the cases of tests/mcl_kld_cases.py; tests/test_mcl_kld.py
holds the twin to the checker and shows on the checker alone that every case does what its name says."""
import numpy as np
import pytest

import mcl_cases as mc
import mcl_kld_cases as kc
import mcl_kld_lib as kl
from visfs_amd import abi, backend, mcl
from visfs_amd import mcl_kld as kld

pytestmark = pytest.mark.gpu

SIZE_CASES = kc.size_cases()
CRAFTED = kc.crafted_cases()


@pytest.fixture(scope="module")
def solver():
    s = backend.Solver(abi.default_params())
    yield s
    s.close()


@pytest.fixture(scope="module")
def rooms(solver):
    cells, lim = mc.room()
    dev, host = mcl.Field.from_grid(cells, lim, solver=solver), mcl.Field.from_grid(cells, lim)
    assert (dev.status, host.status) == (abi.OK, abi.OK)
    yield dev, host
    dev.close(); host.close()


def trace(case, field, device, **kw):
    lib = kl.Library(case, field, **kw)
    limits = lib.limits()
    out = kc.play(case, lib)
    assert lib.counts and all(c == (mcl.UPDATE_COUNTS if device else (0, 0, 0)) for c in lib.counts)     # (4, 2, 1) whatever N, n and the beams
    lib.close()
    return out, limits


def device_equals_twin(rooms, case, **kw):
    (a, la), (b, lb) = trace(case, rooms[0], True, **kw), trace(case, rooms[1], False)
    kl.same(la, lb, "limit")
    kl.same_trace(a, b, (case["name"], kw))
    return a


@pytest.mark.parametrize("case", SIZE_CASES, ids=[c["name"] for c in SIZE_CASES])
def test_sizes_device_equals_twin(rooms, case):
    out = device_equals_twin(rooms, case)
    if case["N"] >= 1023:
        assert out[3][1]["n_before"] < case["N"]                               # updates ran at a count below the capacity
    assert mcl.UPDATE_COUNTS == (4, 2, 1)


def test_the_fullest_table_and_the_capacity_above_it(rooms):
    out = device_equals_twin(rooms, kc.fullest_case())
    assert out[1][0]["resampled"] == 1 and out[1][1]["bins"] > 2000
    f = mcl.Filter(rooms[0], 16385, 1)
    assert f.status == abi.OK and kld.enable(f) == abi.ERR_UNSUPPORTED and kld.count(f) == 16385
    f.close()


@pytest.mark.parametrize("case", CRAFTED, ids=[c["name"] for c in CRAFTED])
def test_crafted_device_equals_twin(rooms, case):
    device_equals_twin(rooms, case)


@pytest.mark.parametrize("kw", [dict(hash_bits=0), dict(hash_bits=3), dict(hash_bits=-1), dict(lanes=1), dict(lanes=64)],
                         ids=["hash_bits_0", "hash_bits_3", "hash_bits_default", "lanes_1", "lanes_64"])
def test_hash_bits_and_lanes_give_the_same_bytes(rooms, kw):
    case = SIZE_CASES[-1]
    assert case["N"] == 1025
    device_equals_twin(rooms, case, **kw)


def test_own_bins_with_every_draw_on_one_home_slot(rooms):
    """The longest probe chains: hundreds of bins that all start at slot 0."""
    case = {c["name"]: c for c in CRAFTED}["own_bins"]
    out = device_equals_twin(rooms, case, hash_bits=0)
    assert out[0][1]["bins"] > 100


def test_a_kld_filter_of_77_equals_a_plain_filter_of_77(rooms):
    kl.check_plain_equality(rooms[0])


def test_life_cycle_on_the_device(rooms):
    kl.check_life_cycle(rooms[0])


def test_the_counts_do_not_depend_on_the_sizes(rooms):
    rng = np.random.default_rng(3)
    for N, n in ((1, 0), (1, 16384), (16384, 0), (16384, 2000)):
        a = mcl.Filter(rooms[0], N, 1)
        assert a.status == abi.OK and kld.enable(a, min_particles=1) == abi.OK
        assert a.init(mc.ROOM_CENTRE, (0.2, 0.2, 0.1)) == abi.OK and a.last_counts() == mcl.INIT_COUNTS
        for _ in range(2):                                                      # one update that skips resampling and one that runs it
            rc, r = a.update((0.1, 0.0, 0.01), mc.cloud(rng, n))
            assert rc == abi.OK and r["n_beams"] == n and a.last_counts() == mcl.UPDATE_COUNTS == (4, 2, 1)
        a.close()


def test_localisation_device_equals_twin(rooms):
    out = device_equals_twin(rooms, kc.localise_case(1))
    ran = [k for r, k, _ in out if r["resampled"]]
    assert len(ran) == 10 and ran[0]["n_after"] == kc.LOCALISE_N and ran[-1]["n_after"] < kc.LOCALISE_N
