"""CPU-only: the refusals of feature_precision= (packed bf16 hash features for forward-only rendering),
word for word. The checkers are called directly, as in test_table_precision_guards.py: nothing here needs a device or
the built library, and every refusal below is raised before anything could be launched."""
import inspect

import pytest
import torch

from indoor_nerf_amd import sparse_field

from test_forward_only_guards import field_modules, refusal

REASON = "the backward reads fp32 features"
NEEDS_BF16 = "feature_precision='bf16' needs mlp_precision='bf16' (the fp32-accurate MLP reads fp32 features)"
FOREIGN = "render_rays: mlp_precision needs a network_query_fn that calls this package's run_network"


def test_reason_is_listed():
    assert sparse_field.NOT_IN_TRAINING["feature_precision"] == REASON
    # the other keywords keep theirs
    assert sparse_field.NOT_IN_TRAINING["mlp_precision"] == "the backward recomputes the forward in fp32"
    assert sparse_field.NOT_IN_TRAINING["table_precision"] == "the backward scatters into the fp32 tables"


@pytest.mark.parametrize("prefix", ["render_rays", "render"])
def test_value_mlp_and_gradients(prefix):
    check = sparse_field.check_feature_precision
    for grad in (torch.no_grad, torch.enable_grad):
        with grad():
            for mlp_bf16 in (False, True):
                # today's path: nothing to refuse, with or without gradients, whatever the MLP
                assert check(None, mlp_bf16, prefix) is False and check("fp32", mlp_bf16, prefix) is False
                for bad in ("fp16", "BF16", "bfloat16", "", 16, True, 0.5, b"bf16", ("bf16",), torch.bfloat16):
                    assert refusal(check, bad, mlp_bf16, prefix) == \
                        f"{prefix}: feature_precision must be None, 'fp32' or 'bf16', got {bad!r}"
            # the MLP is checked before the gradients
            assert refusal(check, "bf16", False, prefix) == f"{prefix}: {NEEDS_BF16}"
    with torch.no_grad():
        assert check("bf16", True, prefix) is True
    with torch.enable_grad():
        assert refusal(check, "bf16", True, prefix) == \
            f"{prefix}: feature_precision is forward-only (call under torch.no_grad(); {REASON})"


def test_literals():
    """The strings as a caller sees them, written out."""
    check = sparse_field.check_feature_precision
    assert refusal(check, "fp16", True, "render") == \
        "render: feature_precision must be None, 'fp32' or 'bf16', got 'fp16'"
    assert refusal(check, "bf16", False, "render_rays") == \
        ("render_rays: feature_precision='bf16' needs mlp_precision='bf16' (the fp32-accurate MLP reads fp32 "
         "features)")
    with torch.enable_grad():
        assert refusal(check, "bf16", True, "render_rays") == \
            ("render_rays: feature_precision is forward-only (call under torch.no_grad(); the backward reads fp32 "
             "features)")


def test_render_rays_and_render_refuse_before_anything_else():
    """Both entry points run the check on their own keywords before they touch the rays: the refusals fire with
    arguments that could not render anything."""
    import indoor_nerf_amd as nerf
    _, net, _, _ = field_modules()
    common = dict(network_fn=net, network_query_fn=None, N_samples=4)
    with torch.no_grad():
        assert refusal(nerf.render_rays, None, feature_precision="bf16", **common) == f"render_rays: {NEEDS_BF16}"
        assert refusal(nerf.render_rays, None, feature_precision="bf16", mlp_precision="fp32", **common) == \
            f"render_rays: {NEEDS_BF16}"
        assert refusal(nerf.render_rays, None, feature_precision="half", mlp_precision="bf16", **common) == \
            "render_rays: feature_precision must be None, 'fp32' or 'bf16', got 'half'"
        assert refusal(nerf.render, 2, 2, None, feature_precision="bf16", **common) == f"render: {NEEDS_BF16}"
        assert refusal(nerf.render, 2, 2, None, feature_precision=16, mlp_precision="bf16", **common) == \
            "render: feature_precision must be None, 'fp32' or 'bf16', got 16"
    with torch.enable_grad():
        # mlp_precision's own refusal comes first: it is the keyword the request rides on
        assert refusal(nerf.render, 2, 2, None, feature_precision="bf16", mlp_precision="bf16", **common) == \
            "render: mlp_precision is forward-only (call under torch.no_grad(); the backward recomputes the forward in fp32)"


def test_request_carries_the_flag():
    """The one request carries it: one attribute on the points for every combination, no global switch."""
    from indoor_nerf_amd.render import _query
    Req = sparse_field.FieldRequest
    pts, seen = torch.zeros(2, 3, 3), []

    def foreign(p, viewdirs, fn):
        seen.append({k: v for k, v in vars(p).items() if k.startswith("_nerf")})
        return torch.zeros(2, 3, 4)

    assert refusal(_query, foreign, pts, None, None, Req(bf16=True, packed=True)) == FOREIGN
    assert list(seen[-1]) == ["_nerf_req"] and seen[-1]["_nerf_req"].packed is True
    assert refusal(_query, foreign, pts, None, None, Req(bf16=True)) == FOREIGN
    assert list(seen[-1]) == ["_nerf_req"] and seen[-1]["_nerf_req"].packed is False
    assert refusal(_query, foreign, pts, None, None, Req(bf16=True, half=True, packed=True)) == \
        "render_rays: table_precision needs a network_query_fn that calls this package's run_network"
    assert list(seen[-1]) == ["_nerf_req"] and seen[-1]["_nerf_req"].packed is True
    for kw in (dict(grid=object()), dict(early=(None, None, 1e-3, 8)), dict(half=True), dict(grid=object(), bf16=True),
               dict(march=sparse_field.MarchList(torch.zeros(2, 16)), bf16=True, half=True, packed=True)):
        refusal(_query, foreign, pts, None, None, Req(**kw))
        assert list(seen[-1]) == ["_nerf_req"], kw
    assert not any(k.startswith("_nerf") for k in vars(pts))
    assert inspect.signature(Req).parameters["packed"].default is False
    assert sparse_field.is_packed(None) is False
    assert sparse_field.is_packed(Req(bf16=True)) is False
    assert sparse_field.is_packed(Req(bf16=True, packed=True)) is True


def test_feature_buffer_halves_the_bytes():
    Req = sparse_field.FieldRequest
    for n in (0, 1, 48):
        buf, w, dt = sparse_field.feature_buffer(None, n, "cpu")
        assert (buf.numel(), w, dt, buf.dtype) == (2 * n, 2, torch.float32, torch.float32)
        buf, w, dt = sparse_field.feature_buffer(Req(bf16=True), n, "cpu")
        assert (buf.numel(), w, dt) == (2 * n, 2, torch.float32)
        pk, w, dt = sparse_field.feature_buffer(Req(bf16=True, packed=True), n, "cpu")
        assert (pk.numel(), w, dt, pk.dtype) == (n, 1, torch.int32, torch.int32)
        assert 2 * pk.numel() * pk.element_size() == buf.numel() * buf.element_size()


def test_encode_into_refuses_active_quantizers():
    """HashEmbedder.encode_into(packed=True) with active A-CAQ quantizers: refused before anything is launched, as
    for half=True."""
    emb_q = field_modules(use_quantization=True)[0].eval()
    assert emb_q.quantization_active()
    xyz, words, keep = torch.zeros(0, 3), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.bool)
    assert refusal(emb_q.encode_into, xyz, words, 1, 0, keep, packed=True) == \
        "encode_into: packed bf16 features are not available with A-CAQ quantizers (the bf16 MLP has no record)"
    assert refusal(emb_q.encode_into, xyz, words, 1, 0, keep, half=True, packed=True) == \
        "encode_into: half tables are not available with A-CAQ quantizers (they have their own packed tables)"


def test_encode_into_checks_the_buffer_in_words():
    """The out-of-range check counts one word per (point, level) entry: a buffer of exactly L * P words passes it
    (and is then refused for being on the CPU), one word less does not."""
    emb = field_modules()[0].eval()
    L_, P = emb.n_levels, 5
    xyz, keep = torch.zeros(P, 3), torch.zeros(P, dtype=torch.bool)
    with torch.no_grad():
        assert refusal(emb.encode_into, xyz, torch.zeros(L_ * P - 1, dtype=torch.int32), 1, P, keep, packed=True) == \
            "encode_into: rows out of the feature / keep buffers"
        with pytest.raises(RuntimeError, match="feat: indoor_nerf_amd kernels need CUDA"):
            emb.encode_into(xyz, torch.zeros(L_ * P, dtype=torch.int32), 1, P, keep, packed=True)
        # unpacked, the same P points need two floats per entry
        assert refusal(emb.encode_into, xyz, torch.zeros(2 * L_ * P - 1), 2, 2 * P, keep) == \
            "encode_into: rows out of the feature / keep buffers"
