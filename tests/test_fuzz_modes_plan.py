"""The inputs of tests/test_gpu_fuzz_modes.py, checked without a GPU: the host-only plan (World.scene_plan, as
tests/test_scene_prep.py::kernel_name reads it) says which ahead-of-time kernel family each seed of the list gets, and the CPU oracle
says what share of each seed's pixels the adaptive threshold flags.  Conditions on the INPUTS: where a change of the generators makes
one fail, the seed list changes (tests/fuzz_modes_helpers.py), not the bound."""
import collections

import numpy as np
import pytest

from tests import fuzz_modes_helpers as FM
from tests.adaptive_helpers import edge_mask


@pytest.fixture(autouse=True)
def _ahead_of_time(monkeypatch):
    import os
    for name in list(os.environ):
        if name.startswith("RTC_AMD_"):
            monkeypatch.delenv(name)
    monkeypatch.setenv("RTC_AMD_SPECIALIZE", "0")


def _families():
    return [(gen, seed, FM.plan_family(gen, seed)) for gen, seed in FM.all_seeds()]


def test_every_ahead_of_time_family_is_there_at_least_twice():
    seen = collections.Counter(f for _, _, f in _families())
    print(dict(seen))
    for family in FM.FAMILIES:
        assert seen[family] >= 2, (family, dict(seen))
    assert set(seen) <= set(FM.FAMILIES), dict(seen)  # a family this file does not know of: name it in FAMILIES


def test_the_seeds_that_also_run_scene_compiled_are_the_first_of_each_family():
    first = {}
    for gen, seed, family in _families():
        first.setdefault(family, (gen, seed))
    assert sorted(FM.SPECIALISED) == sorted(first.values()), first


def test_the_starting_seeds_are_all_there():
    seeds = FM.all_seeds()
    assert len(set(seeds)) == len(seeds)
    for s in list(range(16)) + [2133, 4002, 4003, 9007, 14005]:
        assert ("fuzz", s) in seeds
    for s in range(16):
        assert ("wide", s) in seeds


def test_the_adaptive_thresholds_flag_a_useful_share_of_pixels():
    """Over the whole list at least half the seeds flag between 1 % and 60 % of their pixels (the threshold: the median of the
    nonzero neighbour differences of the oracle's coarse frame, 0.1 where there is none)."""
    shares = {}
    for gen, seed in FM.all_seeds():
        B, _ = FM.oracle_frame(gen, seed, 1)
        shares[gen, seed] = float(edge_mask(B, FM.threshold_of(B)).mean())
    useful = [k for k, v in shares.items() if 0.01 <= v <= 0.60]
    print({k: round(v, 3) for k, v in shares.items()})
    assert 2 * len(useful) >= len(shares), (len(useful), len(shares), shares)


def test_threshold_of():
    B = np.zeros((3, 4, 3), dtype=np.float32)
    assert FM.threshold_of(B) == 0.1
    B[1, 1, 0] = 0.5  # four neighbour pairs differ by 0.5
    assert FM.threshold_of(B) == 0.5
    B[0, 0] = np.nan  # NaN differences are not differences
    assert FM.threshold_of(B) == 0.5
