"""AMCL's pose hypotheses on the GPU (include/visfs_mcl_hyp.h on a device filter: the hypotheses run inside the launch of
k_mcl_kld_resample) against the one-core host twin, byte for byte in the labels, every field of visfs_mcl_hyp_result and everything
tests/test_gpu_mcl_kld.py compares, on the cases of tests/mcl_hyp_cases.py; tests/test_mcl_hyp.py holds the twin to the checker and
shows on the checker alone that every case does what its name says."""
import pytest

import mcl_hyp_cases as hc
import mcl_hyp_lib as hl
import mcl_kld_cases as kc
import mcl_kld_lib as kl
from visfs_amd import abi, backend, mcl

pytestmark = pytest.mark.gpu

SIZE_CASES = hc.size_cases()
CRAFTED = hc.crafted_cases()


@pytest.fixture(scope="module")
def solver():
    s = backend.Solver(abi.default_params())
    yield s
    s.close()


@pytest.fixture(scope="module")
def fields(solver):
    """{world: (the device's field, the twin's)}."""
    out = {w: (hl.field_of(w, solver), hl.field_of(w)) for w in ("room", "box")}
    yield out
    for dev, host in out.values():
        dev.close(); host.close()


def trace(case, field, device, **kw):
    lib = hl.Library(case, field, **kw)
    out = hc.play(case, lib)
    assert lib.counts and all(c == (mcl.UPDATE_COUNTS if device else (0, 0, 0)) for c in lib.counts)     # (4, 2, 1) with the hypotheses too
    lib.close()
    return out, lib.rounds


def device_equals_twin(fields, case, **kw):
    dev, host = fields[case.get("world", "room")]
    (a, rounds), (b, _) = trace(case, dev, True, **kw), trace(case, host, False)
    hl.same_trace(a, b, (case["name"], kw))
    return a, rounds


@pytest.mark.parametrize("case", SIZE_CASES, ids=[c["name"] for c in SIZE_CASES])
def test_sizes_device_equals_twin(fields, case):
    out, _ = device_equals_twin(fields, case)
    assert out[0][3]["fresh"] == 1 and out[0][3]["n"] == case["N"] and mcl.UPDATE_COUNTS == (4, 2, 1)


def test_the_fullest_table(fields):
    out, rounds = device_equals_twin(fields, hc.fullest_case())
    h = out[1][3]
    print(f"N = 16384: {out[1][1]['bins']} bins, {h['n_clusters']} clusters, {rounds[1]} rounds")
    assert out[1][1]["bins"] > 2000 and h["n_clusters"] > 50 and h["n_hypotheses"] == 8


@pytest.mark.parametrize("case", CRAFTED, ids=[c["name"] for c in CRAFTED])
def test_crafted_device_equals_twin(fields, case):
    out, rounds = device_equals_twin(fields, case)
    if case["name"] == "snake":
        print(f"snake: {rounds[0]} rounds")                                    # informational: read, not compared
        assert out[0][3]["hyp"][0]["bins"] == 512
    if case["name"] == "closed_gate":
        assert out[1][0]["resampled"] == 0 and out[1][3] == dict(out[0][3], fresh=0)


@pytest.mark.parametrize("bits", [0, 3, -1], ids=["hash_bits_0", "hash_bits_3", "hash_bits_default"])
def test_hash_bits_give_the_same_bytes(fields, bits):
    for name in ("nine", "spread_N1025"):
        device_equals_twin(fields, hc.all_cases()[name], hash_bits=bits)


def test_hypotheses_off_gives_the_kld_filter(fields):
    """On the device a KLD filter without hypotheses, and one with them, give the twin's KLD trace of tests/mcl_kld_cases.py."""
    case = kc.size_cases()[-1]
    want, _ = trace(case, fields["room"][1], False, hypotheses=False)
    for on in (False, True):
        got, _ = trace(case, fields["room"][0], True, hypotheses=on)
        kl.same_trace([t[:3] for t in got], [t[:3] for t in want], (case["name"], on))


def test_life_cycle_on_the_device(fields):
    hl.check_life_cycle(fields["room"][0])


def test_the_room_device_equals_twin(fields):
    out, rounds = device_equals_twin(fields, hc.room_case(1))
    ran = [(t, r) for t, r in zip(out, rounds) if t[0]["resampled"]]
    print(f"room: rounds {[r for _, r in ran]}")
    assert len(ran) == 10 and all(t[3]["fresh"] == 1 and t[3]["n_hypotheses"] >= 1 for t, _ in ran)


def test_the_mirror_device_equals_twin(fields):
    out, _ = device_equals_twin(fields, hc.mirror_case(hc.MIRROR_SEEDS[0]))
    assert all(t[3]["n_hypotheses"] >= 2 for t in out if t[0]["resampled"])
