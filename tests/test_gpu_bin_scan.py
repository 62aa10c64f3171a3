"""The bin pass's run merge at every form of wave_segmented_inclusive_sum (csrc/common.h): runs of 2..33 copies of
a point starting one lane before, on and after lanes 16, 32 and 48 and one across lanes 63 / 0 (bin_scan_cases.run_set;
test_bin_scan_cpu.py shows which steps each wave takes), at levels 16 and 1024, in the three modes of
test_gpu_hash_bwd_shapes.py against hash_bwd_ref.scatter_ref with that file's bounds; the deterministic mode twice,
bit-identical (needs an MI355X).
"""
import pytest

import bin_scan_cases as bs
import hash_bwd_ref as hb
import test_gpu_hash_bwd_shapes as shapes
from test_gpu_hash_bwd_shapes import ctx  # noqa: F401  (the module fixture of the shapes tests)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", bs.RUN_LENGTHS)
def test_runs_around_row_boundaries(ctx, n):  # noqa: F811
    x, _ = bs.run_set(n)
    assert len(x) <= 2 * ctx.C + 1
    d = hb.random_grads(len(shapes.LEVELS), len(x), seed=300 + n, decades=3.0)
    shapes._all_modes(ctx, f"scan runs of {n}", x, d, levels=shapes.LEVELS, modes=shapes.MODES)
