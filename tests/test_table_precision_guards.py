"""CPU-only: the refusals of table_precision= (the fp16 hash tables of forward-only rendering), word for
word. The checkers are called directly, as in test_mlp_precision_guards.py: nothing here needs a device or the built
library, and every refusal below is raised before anything could be launched."""
import pytest
import torch

from indoor_nerf_amd import sparse_field

from test_forward_only_guards import field_modules, refusal

REASON = "the backward scatters into the fp32 tables"
ACAQ = "A-CAQ quantizers are not supported (they have their own packed tables)"
FOREIGN = "render_rays: table_precision needs a network_query_fn that calls this package's run_network"


def test_reason_is_listed():
    assert sparse_field.NOT_IN_TRAINING["table_precision"] == REASON
    # the other keywords keep theirs
    assert sparse_field.NOT_IN_TRAINING["mlp_precision"] == "the backward recomputes the forward in fp32"


@pytest.mark.parametrize("prefix", ["render_rays", "render"])
def test_value_and_gradients(prefix):
    check = sparse_field.check_table_precision
    for grad in (torch.no_grad, torch.enable_grad):
        with grad():
            # today's path: nothing to refuse, with or without gradients
            assert check(None, prefix) is False and check("fp32", prefix) is False
            for bad in ("bf16", "FP16", "half", "", 16, True, 0.5, b"fp16", ("fp16",), torch.float16):
                assert refusal(check, bad, prefix) == \
                    f"{prefix}: table_precision must be None, 'fp32' or 'fp16', got {bad!r}"
    with torch.no_grad():
        assert check("fp16", prefix) is True
    with torch.enable_grad():
        assert refusal(check, "fp16", prefix) == \
            f"{prefix}: table_precision is forward-only (call under torch.no_grad(); {REASON})"


def test_literals():
    """The strings as a caller sees them, written out."""
    with torch.enable_grad():
        assert refusal(sparse_field.check_table_precision, "fp16", "render_rays") == \
            ("render_rays: table_precision is forward-only (call under torch.no_grad(); the backward scatters into the "
             "fp32 tables)")
    assert refusal(sparse_field.check_table_precision, "bf16", "render") == \
        "render: table_precision must be None, 'fp32' or 'fp16', got 'bf16'"


def test_raw_noise_is_not_refused():
    """The encoding does not care about noise: check_table_precision takes no raw_noise_std at all."""
    import inspect
    assert list(inspect.signature(sparse_field.check_table_precision).parameters) == ["value", "prefix"]
    with torch.no_grad():
        sparse_field.check_forward_only("table_precision", "render_rays")


@pytest.mark.parametrize("prefix", ["render_rays", "render"])
def test_module_refusals(prefix):
    import indoor_nerf_amd as nerf
    emb, net, head, _ = field_modules()
    check = sparse_field.check_table_nets
    check([net], emb, prefix)
    check([net, net], None, prefix)
    check([net, head], emb, prefix)                 # a normals head is allowed: the encoding does not care
    net_q = nerf.NeRFSmall(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64,
                           input_ch=32, input_ch_views=16, use_quantization=True)
    check([net_q], emb, prefix)                     # so is a quantized MLP: its tables are still fp32
    emb_q = field_modules(use_quantization=True)[0]
    assert refusal(check, [net], emb_q, prefix) == f"{prefix}: table_precision: {ACAQ}"
    assert refusal(check, [net, torch.nn.Linear(48, 4)], emb, prefix) == \
        (f"{prefix}: table_precision: needs the fused field modules (HashEmbedder + NeRFSmall), got HashEmbedder + "
         "Linear")
    assert refusal(check, [net], torch.nn.Identity(), prefix) == \
        f"{prefix}: table_precision: needs the fused field modules (HashEmbedder + NeRFSmall), got Identity + NeRFSmall"


def test_default_prefix_is_render_rays():
    emb_q, net = field_modules(use_quantization=True)[:2]
    assert refusal(sparse_field.check_table_nets, [net], emb_q) == f"render_rays: table_precision: {ACAQ}"


def test_field_call_refusals():
    """run_network's own checks of a request on the dense path (a caller's query function may hand it other
    modules than render_rays saw)."""
    emb, net, head, _ = field_modules()
    check, words = sparse_field.check_table_field, "inputs [R, S, 3]"
    with torch.no_grad():
        check(True, words, net, emb)
        check(True, words, head, emb)
        assert refusal(check, False, words, net, emb) == \
            "table_precision: needs the fused field call (SHEncoder view encoding, viewdirs, inputs [R, S, 3])"
        assert refusal(check, True, words, torch.nn.Linear(48, 4), emb) == \
            "table_precision: needs the fused field modules (HashEmbedder + NeRFSmall), got HashEmbedder + Linear"
        emb_q = field_modules(use_quantization=True)[0]
        assert refusal(check, True, words, net, emb_q) == f"table_precision: {ACAQ}"
    with torch.enable_grad():
        assert refusal(check, True, words, net, emb) == \
            f"table_precision: forward-only (call under torch.no_grad(); {REASON})"


def test_encode_into_refuses_active_quantizers():
    """HashEmbedder.encode_into(half=True) with active A-CAQ quantizers: refused before anything is launched or
    allocated (the checks that come first need buffers of the right size only)."""
    emb_q = field_modules(use_quantization=True)[0].eval()
    assert emb_q.quantization_active()
    xyz, feat, keep = torch.zeros(0, 3), torch.zeros(0), torch.zeros(0, dtype=torch.bool)
    assert refusal(emb_q.encode_into, xyz, feat, 2, 0, keep, half=True) == \
        "encode_into: half tables are not available with A-CAQ quantizers (they have their own packed tables)"
    assert emb_q._half is None


def test_run_network_refuses_before_the_eager_path():
    """A request on points that do not make the fused call (no view directions) is refused by run_network itself;
    the request is marked used either way, so render_rays does not blame the query function."""
    import indoor_nerf_amd as nerf
    emb, net, _, sh = field_modules()
    pts = torch.zeros(2, 3, 3)
    req = pts._nerf_req = sparse_field.FieldRequest(half=True)
    assert req.used is False and req.blame == "table_precision"
    with torch.no_grad():
        assert refusal(nerf.run_network, pts, None, net, emb, sh) == \
            "table_precision: needs the fused field call (SHEncoder view encoding, viewdirs, inputs [R, S, 3])"
    assert req.used is True


def test_foreign_query_function_raises():
    """A query function that does not reach this package's run_network leaves the request unused: render_rays'
    field call raises instead of rendering from the fp32 tables. With mlp_precision="bf16" beside it the one request
    carries both, and table_precision is the keyword blamed (FieldRequest.blame: tables before the MLP)."""
    from indoor_nerf_amd.render import _query
    Req = sparse_field.FieldRequest
    pts, seen = torch.zeros(2, 3, 3), []

    def foreign(p, viewdirs, fn):
        seen.append(getattr(p, "_nerf_req", None))
        return torch.zeros(2, 3, 4)

    assert refusal(_query, foreign, pts, None, None, Req(half=True)) == FOREIGN
    assert isinstance(seen[-1], Req) and seen[-1].half is True and seen[-1].bf16 is False
    assert not hasattr(pts, "_nerf_req")
    assert refusal(_query, foreign, pts, None, None, Req(half=True, bf16=False)) == FOREIGN
    assert refusal(_query, foreign, pts, None, None, Req(half=True, bf16=True)) == FOREIGN
    assert seen[-1].half is True and seen[-1].bf16 is True
    assert refusal(_query, foreign, pts, None, None, Req(grid=object(), half=True)) == FOREIGN
    assert refusal(_query, foreign, pts, None, None, req=Req(half=True)) == FOREIGN
    # without the keyword the same function is simply called, with nothing attached
    assert _query(foreign, pts, None, None, None)[0].shape == (2, 3, 4) and seen[-1] is None
    assert _query(foreign, pts, None, None)[0].shape == (2, 3, 4) and seen[-1] is None
    # mlp_precision's own message is unchanged
    assert Req(half=True, bf16=True).blame == "table_precision" and Req(bf16=True).blame == "mlp_precision"
    assert refusal(_query, foreign, pts, None, None, Req(bf16=True)) == \
        "render_rays: mlp_precision needs a network_query_fn that calls this package's run_network"
