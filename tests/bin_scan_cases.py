"""What test_bin_scan_cpu.py and test_gpu_bin_scan.py share: the rule by which wave_segmented_inclusive_sum
(csrc/common.h) picks its steps, an fp32 NumPy emulation of those steps, and the point sets of the GPU test (runs of
copies of one point placed around the 16-lane DPP row boundaries). No test and no fixture lives here.
"""
import numpy as np

import hash_bwd_ref as hb

WAVE, ROW = hb.WAVE, hb.ROW
FULL = 6                                 # the six steps of the classic scan (a run of 17 lanes or more)

RUN_LENGTHS = (2, 3, 4, 5, 8, 9, 15, 16, 17, 33)
# one lane before, on and after lanes 16, 32 and 48; grouped so that one wave holds one placement per boundary
RUN_STARTS = ((15, 31, 47), (16, 32, 48), (17, 33, 49))
MAX_POINTS = 2 * 512 + 1


# ---------------------------------------------------------------- the selection rule
def starts_of(head):
    """First lane of every lane's run from the wave's head flags (lane 0 is always a head)."""
    head = np.asarray(head, bool).copy()
    head[0] = True
    return np.maximum.accumulate(np.where(head, np.arange(WAVE), 0))


def select(start):
    """(steps, carry) the kernel picks for a wave: steps = 0 (no scan), 1..4 intra-row steps, or FULL; carry = the
    single row_bcast:15 step into rows 1-3 (False with FULL, which has the bcast15 / bcast31 pair instead)."""
    lane = np.arange(WAVE)
    span = lane - start
    if not span.any():
        return 0, False
    cross = bool((start < (lane & ~(ROW - 1))).any())
    if span.max() >= 16:
        return FULL, False
    steps = 1 + int(span.max() >= 2) + int(span.max() >= 4) + int(span.max() >= 8)
    return steps, cross


def wave_variants(base, n_valid=None):
    """select() for every wave of 64 points, from the voxel bases (invalid lanes of a ragged last wave form one run,
    as in hash_bwd_ref.wave_scan_variants)."""
    base = np.asarray(base)
    P = len(base) if n_valid is None else n_valid
    out = []
    for w0 in range(0, P, WAVE):
        b = base[w0:min(w0 + WAVE, P)]
        n = len(b)
        head = np.ones(WAVE, bool)
        head[1:n] = (b[1:] != b[:-1]).any(-1)
        head[n + 1:] = False
        out.append(select(starts_of(head)))
    return out


# ---------------------------------------------------------------- fp32 emulation of the DPP steps
def _src_row_shr(n):
    lane = np.arange(WAVE)
    return np.where((lane & (ROW - 1)) >= n, lane - n, -1)


def _src_bcast15(row_mask):
    lane = np.arange(WAVE)
    row = lane // ROW
    ok = (row >= 1) & (((row_mask >> row) & 1) == 1)
    return np.where(ok, ROW * row - 1, -1)


def _src_bcast31(row_mask):
    lane = np.arange(WAVE)
    row = lane // ROW
    ok = (row >= 2) & (((row_mask >> row) & 1) == 1)
    return np.where(ok, 31, -1)


def _step(v, src, take):
    """seg_scan_step: t = v + (the source lane's v, read before any lane writes), kept where `take`. Lanes without a
    source never take the step (asserted), so what they would read does not matter."""
    assert not (take & (src < 0)).any()
    t = (v + v[np.maximum(src, 0)]).astype(np.float32)
    return np.where(take[:, None], t, v)


def _intra(v, start, steps):
    lane = np.arange(WAVE)
    r16, span = lane & (ROW - 1), lane - start
    for k in range(steps):
        d = 1 << k
        v = _step(v, _src_row_shr(d), (r16 >= d) & (span >= d))
    return v


def scan_full(v, start):
    """The six steps: row_shr 1, 2, 4, 8, row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3."""
    lane = np.arange(WAVE)
    row = lane // ROW
    v = _intra(np.asarray(v, np.float32), start, 4)
    v = _step(v, _src_bcast15(0xA), ((row & 1) == 1) & (start <= ROW * row - 1))
    return _step(v, _src_bcast31(0xC), (row >= 2) & (start <= 31))


def scan_selected(v, start):
    """What the kernel runs: the steps select() picks."""
    steps, carry = select(start)
    v = np.asarray(v, np.float32)
    if steps == 0:
        return v
    if steps == FULL:
        return scan_full(v, start)
    v = _intra(v, start, steps)
    if carry:
        lane = np.arange(WAVE)
        v = _step(v, _src_bcast15(0xF), start < (lane & ~(ROW - 1)))      # row 0 has no source and never takes it
    return v


def scan_exact(v, start):
    """Segmented inclusive sums in float64, lane by lane."""
    v = np.asarray(v, np.float64)
    out = v.copy()
    for lane in range(1, WAVE):
        if start[lane] < lane:
            out[lane] = out[lane - 1] + v[lane]
    return out


# ---------------------------------------------------------------- the GPU test's point sets
def run_set(n, seed=17):
    """Runs of n copies of one point starting at every lane of RUN_STARTS, then one run of n across the lanes 63 / 0
    of two waves, then a wave and a point of single points: (xyz [P, 3] fp32, table rows (start point, length)).
    Single points pad up to each start; every run and every single has its own coarse cell (hash_bwd_ref._cell_point),
    so neighbours never merge at any level."""
    rng = np.random.RandomState(seed + n)
    pts, table = [], []
    count = [0, 0]                          # points, cells

    def add(m, record=False):
        if record:
            table.append((count[0], m))
        pts.append(np.repeat(hb._cell_point(rng, 37 * count[1] + 5)[None], m, 0))
        count[0] += m
        count[1] += 1

    def pad_to(lane):
        while count[0] % WAVE != lane:
            add(1)

    for group in RUN_STARTS:
        for s in group:
            if count[0] % WAVE > s:
                pad_to(0)
            pad_to(s)
            add(n, True)
        pad_to(0)
    pad_to(WAVE - (n + 1) // 2)
    add(n, True)                            # across the wave boundary: the merge must break it there
    pad_to(0)
    for _ in range(WAVE + 1):
        add(1)
    x = np.concatenate(pts).astype(np.float32)
    assert len(x) <= MAX_POINTS, len(x)
    return x, np.asarray(table, np.int64)
