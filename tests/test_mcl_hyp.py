"""AMCL's pose hypotheses on the KLD filter (include/visfs_mcl_hyp.h) on the CPU: the one-core host twin
against the checker of tests/mcl_hyp_oracle.py, byte for byte in the labels, every field of visfs_mcl_hyp_result and everything
tests/test_mcl_kld.py compares, on the cases of tests/mcl_hyp_cases.py.  Before the library is compared, the checker's output alone
must show that each case does what its name says.  tests/test_gpu_mcl_hyp.py holds the device to the twin."""
import functools

import pytest

import mcl_cases as mc
import mcl_hyp_cases as hc
import mcl_hyp_lib as hl
import mcl_hyp_oracle as ho
import mcl_kld_cases as kc
import mcl_kld_lib as kl
from visfs_amd import abi, mcl
from visfs_amd import mcl_hyp as hyp
from visfs_amd import mcl_kld as kld

SIZE_CASES = hc.size_cases()
CRAFTED = hc.crafted_cases()


@functools.lru_cache(maxsize=None)
def twin_field(world="room"):
    return hl.field_of(world)


def twin_trace(case, **kw):
    lib = hl.Library(case, twin_field(case.get("world", "room")), **kw)
    out = hc.play(case, lib)
    assert lib.counts and all(c == (0, 0, 0) for c in lib.counts)             # the twin issues nothing
    assert not any(lib.rounds)                                                # ... and runs no rounds
    lib.close()
    return out


def test_the_abi_and_the_struct():
    assert hyp.load().visfs_mcl_hyp_abi_version() == hyp.ABI_VERSION == 1
    assert kld.load().visfs_mcl_kld_abi_version() == 1 and mcl.load().visfs_mcl_abi_version() == 1
    import ctypes
    assert ctypes.sizeof(hyp.Hypothesis) == 16 + 8 * 13 and ctypes.sizeof(hyp.Result) == 24 + hyp.HYP_MAX * ctypes.sizeof(hyp.Hypothesis)
    assert hyp.HYP_MAX == ho.HYP_MAX == 8


@pytest.mark.parametrize("case", SIZE_CASES, ids=[c["name"] for c in SIZE_CASES])
def test_sizes_twin_equals_checker(case):
    hc.check_case(case["name"])
    hl.same_trace(twin_trace(case), hc.reference(case["name"]), case["name"])


def test_the_fullest_table():
    case = hc.fullest_case()
    hc.check_case(case["name"])
    hl.same_trace(twin_trace(case), hc.reference(case["name"]), case["name"])


@pytest.mark.parametrize("case", CRAFTED, ids=[c["name"] for c in CRAFTED])
def test_crafted_twin_equals_checker(case):
    hc.check_case(case["name"])
    hl.same_trace(twin_trace(case), hc.reference(case["name"]), case["name"])


def test_hash_bits_leave_the_twin_alone():
    case = {c["name"]: c for c in CRAFTED}["nine"]
    for bits in (0, 3):
        hl.same_trace(twin_trace(case, hash_bits=bits), hc.reference(case["name"]), bits)


def test_hypotheses_off_gives_the_kld_filter():
    """A KLD filter without hypotheses gives the checker's KLD trace of tests/mcl_kld_cases.py, and so does one with them."""
    case = kc.size_cases()[-1]
    ref = kc.reference(case["name"])
    for on in (False, True):
        got = twin_trace(case, hypotheses=on)
        kl.same_trace([t[:3] for t in got], ref, (case["name"], on))


def test_life_cycle_on_the_twin():
    hl.check_life_cycle(twin_field())


# ---------------------------------------------------------------- the localisation scenes, on the checker
def test_the_room_hypothesis_0_localises():
    for seed, measured in zip(hc.LOCALISE_SEEDS, hc.ROOM_MEASURED):
        et, er = hc.room_errors(seed)
        ref = hc.reference(f"room_seed{seed}")
        print(f"seed {seed}: hypothesis 0 final error {et:.4f} m, {er:.4f} rad (measured {measured}); clusters {[t[3]['n_clusters'] for t in ref if t[0]['resampled']]}")
        assert et <= hc.ROOM_BOUND[0] and er <= hc.ROOM_BOUND[1], (seed, et, er)
    case = hc.room_case(1)
    hl.same_trace(twin_trace(case), hc.reference(case["name"]), "room seed 1")


def test_the_mirror_keeps_both_hypotheses():
    for seed in hc.MIRROR_SEEDS:
        hc.check_mirror(seed)
    case = hc.mirror_case(hc.MIRROR_SEEDS[0])
    hl.same_trace(twin_trace(case), hc.reference(case["name"]), case["name"])
