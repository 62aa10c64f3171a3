"""CPU-only: the refusals of the forward-only render paths (occupancy=, early_stop=, ray_bounds=, march=;
DESIGN.md §13-§16), word for word. The checkers are called directly: nothing here needs a device or the built
library, and every refusal below is raised before anything could be launched."""
import pytest
import torch

from indoor_nerf_amd import early_stop, occupancy, sparse_field

REASON = {"occupancy": "the grid is not used in training", "early_stop": "rays are not stopped in training",
          "march": "rays are not marched in training", "ray_bounds": "rays are not bounded in training"}
PREFIX = {"occupancy": "render_rays", "early_stop": "render_rays", "march": "render_rays", "ray_bounds": "render"}
NORMALS = ("a normals head is not supported (run_network's box mask then lands on n_z, not on sigma, so a skipped "
           "sample is not a zero-weight sample)")
BBOX = (torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0]))


def refusal(fn, *args, **kwargs):
    with pytest.raises(ValueError) as e:
        fn(*args, **kwargs)
    return str(e.value)


@pytest.mark.parametrize("what", list(REASON))
def test_keyword_guard(what):
    prefix = PREFIX[what]
    with torch.enable_grad():
        assert refusal(sparse_field.check_forward_only, what, prefix) == \
            f"{prefix}: {what} is forward-only (call under torch.no_grad(); {REASON[what]})"
        # gradients are refused before noise
        assert refusal(sparse_field.check_forward_only, what, prefix, 1.0).endswith(f"{REASON[what]})")
    with torch.no_grad():
        assert refusal(sparse_field.check_forward_only, what, prefix, raw_noise_std=1.0) == \
            f"{prefix}: {what} needs raw_noise_std == 0 (noise makes relu(sigma + noise) > 0 at skipped samples)"
        sparse_field.check_forward_only(what, prefix)
        sparse_field.check_forward_only(what, prefix, 0.0)


def test_keyword_guard_literals():
    """The four strings as a caller sees them, written out."""
    with torch.enable_grad():
        got = [refusal(sparse_field.check_forward_only, w, PREFIX[w]) for w in REASON]
    assert got == [
        "render_rays: occupancy is forward-only (call under torch.no_grad(); the grid is not used in training)",
        "render_rays: early_stop is forward-only (call under torch.no_grad(); rays are not stopped in training)",
        "render_rays: march is forward-only (call under torch.no_grad(); rays are not marched in training)",
        "render: ray_bounds is forward-only (call under torch.no_grad(); rays are not bounded in training)"]
    with torch.no_grad():
        got = [refusal(sparse_field.check_forward_only, w, "render_rays", 1.0) for w in ("occupancy", "early_stop", "march")]
    assert got == [
        "render_rays: occupancy needs raw_noise_std == 0 (noise makes relu(sigma + noise) > 0 at skipped samples)",
        "render_rays: early_stop needs raw_noise_std == 0 (noise makes relu(sigma + noise) > 0 at skipped samples)",
        "render_rays: march needs raw_noise_std == 0 (noise makes relu(sigma + noise) > 0 at skipped samples)"]


def field_modules(**emb_kw):
    import indoor_nerf_amd as nerf
    net = dict(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64, input_ch=32,
               input_ch_views=16)
    return (nerf.HashEmbedder(BBOX, log2_hashmap_size=4, finest_resolution=32, **emb_kw), nerf.NeRFSmall(**net),
            nerf.NeRFSmall(predict_normals=True, **net), nerf.SHEncoder())


@pytest.mark.parametrize("what,words", [("occupancy", "inputs [R, S, 3]"), ("early_stop", "inputs [R, S, 3]"),
                                        ("march", "packed inputs [n, 3]")])
def test_field_call_refusals(what, words):
    emb, net, head, sh = field_modules()
    begin, dirs = sparse_field._begin_field_call, torch.zeros(1, 3)
    fused = f"{what}: needs the fused field call (SHEncoder view encoding, viewdirs, {words})"
    with torch.no_grad():
        assert refusal(begin, what, True, words, dirs, net, emb, torch.nn.Identity()) == fused
        assert refusal(begin, what, True, words, None, net, emb, sh) == fused
        assert refusal(begin, what, False, words, dirs, net, emb, sh) == fused
        assert refusal(begin, what, True, words, dirs, torch.nn.Linear(48, 4), emb, sh) == \
            f"{what}: needs the fused field modules (HashEmbedder + NeRFSmall), got HashEmbedder + Linear"
        emb_q = field_modules(use_quantization=True)[0]
        assert refusal(begin, what, True, words, dirs, net, emb_q, sh) == \
            (f"{what}: A-CAQ quantizers are not supported (fp32 tables and weights only: the activation calibration "
             "depends on which points come first)")
        assert refusal(begin, what, True, words, dirs, head, emb, sh) == f"{what}: {NORMALS}"
    with torch.enable_grad():
        assert refusal(begin, what, True, words, dirs, net, emb, sh) == \
            f"{what}: forward-only (call under torch.no_grad(); {REASON[what]})"
    # a refused call leaves the step count alone; an accepted one counts a training-mode encoder's step only
    step = emb.current_step
    with torch.no_grad():
        begin(what, True, words, dirs, net, emb, sh)
        assert emb.current_step == step + 1
        emb.eval()
        begin(what, True, words, dirs, net, emb, sh)
        assert emb.current_step == step + 1


@pytest.mark.parametrize("method", ["ray_span", "march"])
def test_packed_rows(method):
    words = f"OccupancyGrid.{method}: rays must be packed rows [R, 8] or [R, 11] (o, d, near, far[, viewdir]), got "
    assert refusal(occupancy._packed_rows, [[0.0] * 8], method) == words + "list"
    assert refusal(occupancy._packed_rows, torch.zeros(8), method) == words + "(8,)"
    assert refusal(occupancy._packed_rows, torch.zeros(5, 9), method) == words + "(5, 9)"
    for cols in (8, 11):
        rows = torch.zeros(5, 2 * cols, dtype=torch.float64, requires_grad=True)[:, ::2]
        got = occupancy._packed_rows(rows, method)
        assert got.shape == (5, cols) and got.dtype == torch.float32 and got.is_contiguous() and not got.requires_grad


def test_march_parameter_checks():
    for bad in (0, 4097, 2.5, True, "8"):
        for what in ("render_rays: march", "OccupancyGrid.march"):
            assert refusal(occupancy.check_march_samples, bad, what) == \
                f"{what}: march_samples must be an integer in 1..4096, got {bad!r}"
    assert [occupancy.check_march_samples(k, "x") for k in (1, 4096)] == [1, 4096]
    for bad in (0, -1, 2.5, True):
        assert refusal(sparse_field.check_march_points, bad) == \
            f"march: march_points must be a positive integer, got {bad!r}"
    big = 2 ** 27 - 32
    assert refusal(sparse_field.check_march_points, big) == \
        f"march: march_points {big} exceeds the MLP's 32-bit row indexing (16 (n + 32) < 2^31)"
    assert sparse_field.check_march_points(big - 1) == big - 1


def test_early_stop_parameter_checks():
    for bad in (0.0, 1.0, -0.5, 2.0, float("nan")):
        assert refusal(early_stop.check_params, bad, 32) == \
            f"render_rays: early_stop must be a transmittance threshold in (0, 1), got {bad}"
    for bad in (0, -3, 2.5):
        assert refusal(early_stop.check_params, 1e-3, bad) == \
            f"render_rays: early_stop_slab must be an integer >= 1, got {bad}"
    assert early_stop.check_params(1e-3, 32.0) == (1e-3, 32)
