"""Early ray termination for forward-only rendering.

render_rays(..., early_stop=eps) runs each field call front to back in slabs of early_stop_slab samples
(sparse_field.run_network_sparse): the samples of the rays still alive — inside the box and, with an occupancy
grid, in an occupied cell — are compacted in ascending order (csrc/sparse_points.hip), hash-encoded and run
through the MLP; after every slab but the last each ray alive adds the slab to its optical depth and dies
for all later slabs once tau > -log(eps). A sample of a dead ray gets an all-zero raw row, exactly as a
sample the grid skips, so the composited maps are the dense ones with sigma masked per sample, and each
pass differs from its unmasked self by at most eps per channel.

    render_kwargs_test["early_stop"] = 1e-3             # render / render_path stop rays at T < 1e-3
    render_kwargs_test["occupancy"] = grid               # optional: composes with an OccupancyGrid

Forward-only, with the occupancy path's refusals (occupancy.py).
"""
import math

import numpy as np

_LAST = {"counts": (0, 0)}


def last_counts():
    """(points evaluated, points total) of the most recent field call, summed over its slabs."""
    return _LAST["counts"]


def check_params(early_stop, early_stop_slab):
    """(eps, K) of render_rays' keyword arguments, or ValueError."""
    eps = float(early_stop)
    if not 0.0 < eps < 1.0:
        raise ValueError(f"render_rays: early_stop must be a transmittance threshold in (0, 1), got {early_stop}")
    if int(early_stop_slab) != early_stop_slab or int(early_stop_slab) < 1:
        raise ValueError(f"render_rays: early_stop_slab must be an integer >= 1, got {early_stop_slab}")
    return eps, int(early_stop_slab)


def tau_max_of(eps):
    """float32(-log(eps)): the logarithm in double on the host, rounded once."""
    return float(np.float32(-math.log(eps)))
