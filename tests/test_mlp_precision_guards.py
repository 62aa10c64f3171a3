"""CPU-only: the refusals of mlp_precision= (the bf16 MLP forward of forward-only rendering), word for
word. The checkers are called directly, as in test_forward_only_guards.py: nothing here needs a device or the built
library, and every refusal below is raised before anything could be launched."""
import pytest
import torch

from indoor_nerf_amd import sparse_field

from test_forward_only_guards import field_modules, refusal

REASON = "the backward recomputes the forward in fp32"
ACAQ = ("A-CAQ quantizers are not supported (fp32 tables and weights only: the activation calibration depends on "
        "which points come first)")


def test_reason_is_listed():
    assert sparse_field.NOT_IN_TRAINING["mlp_precision"] == REASON


@pytest.mark.parametrize("prefix", ["render_rays", "render"])
def test_value_and_gradients(prefix):
    check = sparse_field.check_mlp_precision
    for grad in (torch.no_grad, torch.enable_grad):
        with grad():
            # today's path: nothing to refuse, with or without gradients
            assert check(None, prefix) is False and check("fp32", prefix) is False
            for bad in ("fp16", "BF16", "", 16, True, 0.5, b"bf16", ("bf16",)):
                assert refusal(check, bad, prefix) == \
                    f"{prefix}: mlp_precision must be None, 'fp32' or 'bf16', got {bad!r}"
    with torch.no_grad():
        assert check("bf16", prefix) is True
    with torch.enable_grad():
        assert refusal(check, "bf16", prefix) == \
            f"{prefix}: mlp_precision is forward-only (call under torch.no_grad(); {REASON})"


def test_literals():
    """The strings as a caller sees them, written out."""
    with torch.enable_grad():
        assert refusal(sparse_field.check_mlp_precision, "bf16", "render_rays") == \
            ("render_rays: mlp_precision is forward-only (call under torch.no_grad(); the backward recomputes the "
             "forward in fp32)")
    assert refusal(sparse_field.check_mlp_precision, "half", "render") == \
        "render: mlp_precision must be None, 'fp32' or 'bf16', got 'half'"


def test_raw_noise_is_not_refused():
    """Noise is added after the field: check_mlp_precision takes no raw_noise_std at all, and render_rays passes
    none to check_forward_only for this keyword."""
    import inspect
    assert list(inspect.signature(sparse_field.check_mlp_precision).parameters) == ["value", "prefix"]
    with torch.no_grad():
        sparse_field.check_forward_only("mlp_precision", "render_rays")


def test_render_rays_module_refusals():
    emb, net, head, _ = field_modules()
    check = sparse_field.check_mlp_nets
    normals = "render_rays: mlp_precision does not support predict_normals or a normals head"
    check([net], emb, False)
    check([net, net], None, False)
    assert refusal(check, [net], emb, True) == normals
    assert refusal(check, [head], emb, False) == normals
    assert refusal(check, [net, head], emb, False) == normals        # the fine network's head, before the coarse pass
    emb_q = field_modules(use_quantization=True)[0]
    assert refusal(check, [net], emb_q, False) == f"render_rays: mlp_precision: {ACAQ}"
    import indoor_nerf_amd as nerf
    net_q = nerf.NeRFSmall(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64,
                           input_ch=32, input_ch_views=16, use_quantization=True)
    assert refusal(check, [net, net_q], emb, False) == f"render_rays: mlp_precision: {ACAQ}"
    assert refusal(check, [torch.nn.Linear(48, 4)], emb, False) == \
        ("render_rays: mlp_precision: needs the fused field modules (HashEmbedder + NeRFSmall), got HashEmbedder + "
         "Linear")


def test_field_call_refusals():
    """run_network's own checks of a request on the dense path (a caller's query function may hand it other
    modules than render_rays saw)."""
    emb, net, head, _ = field_modules()
    check, words = sparse_field.check_mlp_field, "inputs [R, S, 3]"
    with torch.no_grad():
        check(True, words, net, emb)
        assert refusal(check, False, words, net, emb) == \
            "mlp_precision: needs the fused field call (SHEncoder view encoding, viewdirs, inputs [R, S, 3])"
        assert refusal(check, True, words, torch.nn.Linear(48, 4), emb) == \
            "mlp_precision: needs the fused field modules (HashEmbedder + NeRFSmall), got HashEmbedder + Linear"
        emb_q = field_modules(use_quantization=True)[0]
        assert refusal(check, True, words, net, emb_q) == f"mlp_precision: {ACAQ}"
        assert refusal(check, True, words, head, emb) == \
            "mlp_precision: a normals head is not supported (the bf16 forward has no geo output)"
    with torch.enable_grad():
        assert refusal(check, True, words, net, emb) == \
            f"mlp_precision: forward-only (call under torch.no_grad(); {REASON})"


def test_run_network_refuses_before_the_eager_path():
    """A request on points that do not make the fused call (no view directions) is refused by run_network itself;
    the request is marked used either way, so render_rays does not blame the query function."""
    import indoor_nerf_amd as nerf
    emb, net, _, sh = field_modules()
    pts = torch.zeros(2, 3, 3)
    req = pts._nerf_req = sparse_field.FieldRequest(bf16=True)
    assert req.used is False
    with torch.no_grad():
        assert refusal(nerf.run_network, pts, None, net, emb, sh) == \
            "mlp_precision: needs the fused field call (SHEncoder view encoding, viewdirs, inputs [R, S, 3])"
    assert req.used is True


def test_foreign_query_function_raises():
    """A query function that does not reach this package's run_network leaves the request unused: render_rays'
    field call raises instead of returning an fp32 render."""
    from indoor_nerf_amd.render import _query
    pts, seen = torch.zeros(2, 3, 3), []

    def foreign(p, viewdirs, fn):
        seen.append(getattr(p, "_nerf_req", None))
        return torch.zeros(2, 3, 4)

    words = "render_rays: mlp_precision needs a network_query_fn that calls this package's run_network"
    req = sparse_field.FieldRequest(bf16=True)
    assert refusal(_query, foreign, pts, None, None, req) == words
    assert seen[0] is req and req.bf16 is True and not hasattr(pts, "_nerf_req")
    assert refusal(_query, foreign, pts, None, None, req=sparse_field.FieldRequest(bf16=True)) == words
    # without the keyword the same function is simply called, with nothing attached
    raw, stops = _query(foreign, pts, None, None, None)
    assert raw.shape == (2, 3, 4) and stops is None and seen[-1] is None
    assert _query(foreign, pts, None, None)[0].shape == (2, 3, 4) and seen[-1] is None
