"""The step selection of wave_segmented_inclusive_sum (csrc/common.h), on the CPU: an fp32 NumPy emulation of the
DPP steps over 64 lanes x 16 values (bin_scan_cases.py) shows that the steps the kernel picks for a wave — 1..4
intra-row steps by the longest span, plus one row_bcast:15 carry into rows 1-3 where a run crosses a row — give the
sums of the full six steps bit for bit whenever every run is shorter than 17 lanes, and that the point sets of
test_gpu_bin_scan.py reach every form.
"""
import itertools

import numpy as np
import pytest

import bin_scan_cases as bs
import hash_bwd_ref as hb

WAVE, ROW, FULL = bs.WAVE, bs.ROW, bs.FULL
NV = 16                                   # values per lane: 8 corners x 2 features


def _values(rng, decades=6.0):
    v = rng.randn(WAVE, NV) * 10.0 ** rng.uniform(-decades, 0, (WAVE, NV))
    return v.astype(np.float32)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _heads_of_runs(runs):
    """Head flags of a wave of single lanes with the runs (start, length) laid over them."""
    head = np.ones(WAVE, bool)
    for s, n in runs:
        head[s + 1:min(s + n, WAVE)] = False
    return head


def _check(head, v):
    start = bs.starts_of(head)
    full, got = bs.scan_full(v, start), bs.scan_selected(v, start)
    assert _same_bits(full, got), (bs.select(start), np.flatnonzero(head))
    return start


def test_emulation_sums_the_runs():
    """The emulated full scan is a segmented inclusive sum: exact on small integers, any run lengths."""
    rng = np.random.RandomState(1)
    for _ in range(200):
        head = rng.rand(WAVE) < rng.choice([0.05, 0.2, 0.5, 0.8])
        start = bs.starts_of(head)
        v = rng.randint(-64, 65, (WAVE, NV)).astype(np.float32)
        want = bs.scan_exact(v, start)
        assert np.array_equal(bs.scan_full(v, start).astype(np.float64), want)
        assert np.array_equal(bs.scan_selected(v, start).astype(np.float64), want)


def test_single_run_every_start_and_length():
    """One run of 2..16 lanes at every start lane (cut at lane 63), the other lanes single: the selected steps equal
    the six, and the form is the one the longest span and the crossing ask for."""
    rng = np.random.RandomState(2)
    seen_start, ends_at_63 = set(), 0
    for s, n in itertools.product(range(WAVE - 1), range(2, 17)):
        head = _heads_of_runs([(s, n)])
        start = _check(head, _values(rng))
        last = min(s + n, WAVE) - 1
        span = last - s
        steps, carry = bs.select(start)
        assert steps == 1 + (span >= 2) + (span >= 4) + (span >= 8)
        assert carry == (s // ROW != last // ROW)
        seen_start.add(s)
        ends_at_63 += last == WAVE - 1
    assert {14, 15, 16, 30, 31, 32, 46, 47, 48} <= seen_start
    assert ends_at_63 >= 15


@pytest.mark.parametrize("boundary", [16, 32, 48])
def test_every_layout_around_a_row_boundary(boundary):
    """All 2^11 head patterns of the 11 lanes boundary-5 .. boundary+5 (runs of up to 12 lanes in every position
    across the boundary), the rest of the wave single lanes or random short runs."""
    rng = np.random.RandomState(boundary)
    lanes = np.arange(boundary - 5, boundary + 6)
    forms = set()
    for bits in range(1 << len(lanes)):
        head = rng.rand(WAVE) < rng.choice([0.6, 2.0])
        head[lanes] = (bits >> np.arange(len(lanes))) & 1
        head[lanes[0] - 1] = head[lanes[-1] + 1] = True
        start = bs.starts_of(head)
        if (np.arange(WAVE) - start).max() >= 16:
            continue
        _check(head, _values(rng))
        forms.add(bs.select(start))
    assert {(s, c) for s in (1, 2, 3, 4) for c in (False, True)} <= forms


def test_random_layouts_of_short_runs():
    """Random waves whose runs are all shorter than 17 lanes, among them runs that end at lane 63 and runs through
    two boundaries' neighbourhoods (15-31, 31-47)."""
    rng = np.random.RandomState(3)
    forms, n = set(), 0
    while n < 3000:
        head = rng.rand(WAVE) < rng.choice([0.1, 0.15, 0.3, 0.5, 0.9])
        start = bs.starts_of(head)
        if (np.arange(WAVE) - start).max() >= 16:
            continue
        n += 1
        _check(head, _values(rng, decades=rng.choice([0.0, 6.0, 12.0])))
        forms.add(bs.select(start))
    assert {(s, True) for s in (1, 2, 3, 4)} <= forms
    for runs in ([(15, 16), (31, 16), (47, 16)], [(0, 16), (16, 16), (32, 16), (48, 16)], [(14, 3), (30, 3), (46, 3)],
                 [(15, 2), (31, 2), (47, 2), (62, 2)], [(1, 16), (17, 16), (33, 16), (49, 15)], [(48, 16)], [(60, 4)]):
        start = _check(_heads_of_runs(runs), _values(rng))
        assert bs.select(start)[0] != FULL


def test_long_runs_take_the_full_form():
    """A run of 17 lanes or more anywhere selects the six steps (whatever else the wave holds); 16 lanes do not."""
    rng = np.random.RandomState(4)
    for s, n in itertools.product(range(WAVE - 16), (17, 18, 31, 33, 64)):
        head = rng.rand(WAVE) < 0.5
        head[s] = True
        head[s + 1:min(s + n, WAVE)] = False
        start = bs.starts_of(head)
        assert bs.select(start) == (FULL, False)
        v = rng.randint(-64, 65, (WAVE, NV)).astype(np.float32)
        assert np.array_equal(bs.scan_selected(v, start).astype(np.float64), bs.scan_exact(v, start))
    for s in range(WAVE - 15):
        assert bs.select(bs.starts_of(_heads_of_runs([(s, 16)])))[0] == 4
    assert bs.select(bs.starts_of(np.ones(WAVE, bool))) == (0, False)


def test_old_rule_took_the_full_form_where_the_new_one_does_not(oracle):
    """hash_bwd_ref.wave_scan_variants states the rule before this one: every wave with a crossing run took the six
    steps. On the GPU test's sets the new rule takes them only for runs of 17 and 33."""
    for n in bs.RUN_LENGTHS:
        x, _ = bs.run_set(n)
        base = hb.cells(oracle, x, 1024.0)
        old = hb.wave_scan_variants(base)
        new = bs.wave_variants(base)
        assert len(old) == len(new)
        for o, (steps, carry) in zip(old, new):
            if carry or steps >= 3:
                assert o == 4
            else:
                assert o == steps
        assert any(steps == FULL for steps, _ in new[:-1]) == (n >= 17)      # the last, ragged wave aside


def test_gpu_sets_reach_every_form(oracle):
    """The point sets of test_gpu_bin_scan.py: the run table is what the merge sees at both levels, the runs start
    one lane before, on and after lanes 16, 32 and 48 and one crosses lanes 63 / 0, and over all sets the waves take
    every form: 1..4 steps with and without the carry, the six steps, and no scan."""
    forms = set()
    for n in bs.RUN_LENGTHS:
        x, table = bs.run_set(n)
        assert len(x) <= bs.MAX_POINTS
        for r in (16.0, 1024.0):
            base = hb.cells(oracle, x, r)
            runs = hb.runs_of(base)
            assert {tuple(t) for t in table} == {tuple(t) for t in runs[runs[:, 1] > 1]}
            assert (runs[runs[:, 1] > 1][:, 1] == n).all()
            forms |= set(bs.wave_variants(base))
        lanes = table[:, 0] % WAVE
        assert sorted(lanes[:9]) == sorted(s for g in bs.RUN_STARTS for s in g)
        assert len(table) == 10 and lanes[9] + n > WAVE          # the last run leaves its wave
    want = {(s, c) for s in (1, 2, 3, 4) for c in (False, True)} | {(FULL, False), (0, False)}
    assert want <= forms, want - forms
