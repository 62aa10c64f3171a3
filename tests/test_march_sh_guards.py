"""CPU-only: the refusals of march_sh= (SH read through a ray index in the grid march), word for word,
the request that carries the index, and the one place that chooses the MLP entry. The checkers are called directly,
as in test_feature_precision_guards.py: nothing here needs a device or the built library, and every refusal below is
raised before anything could be launched."""
import pytest
import torch

from indoor_nerf_amd import sparse_field

from test_forward_only_guards import field_modules, refusal

REASON = "the backward reads per-point SH rows"
NEEDS_MARCH = "march_sh='rays' needs march= (the ray index belongs to a grid march's list)"
GRID = object()      # check_march_sh only asks whether march= was given


def test_reason_is_listed():
    assert sparse_field.NOT_IN_TRAINING["march_sh"] == REASON
    assert sparse_field.NOT_IN_TRAINING["march"] == "rays are not marched in training"      # the others keep theirs
    assert sparse_field.NOT_IN_TRAINING["feature_precision"] == "the backward reads fp32 features"


@pytest.mark.parametrize("prefix", ["render_rays", "render"])
def test_value_march_and_gradients(prefix):
    check = sparse_field.check_march_sh
    for grad in (torch.no_grad, torch.enable_grad):
        with grad():
            for march in (None, GRID):
                # today's path: nothing to refuse, with or without gradients or a march
                assert check(None, march, prefix) is False and check("rows", march, prefix) is False
                for bad in ("ray", "RAYS", "row", "", 1, True, 0.5, b"rays", ("rays",), torch.int32):
                    assert refusal(check, bad, march, prefix) == \
                        f"{prefix}: march_sh must be None, 'rows' or 'rays', got {bad!r}"
            # the march is checked before the gradients
            assert refusal(check, "rays", None, prefix) == f"{prefix}: {NEEDS_MARCH}"
    with torch.no_grad():
        assert check("rays", GRID, prefix) is True
    with torch.enable_grad():
        assert refusal(check, "rays", GRID, prefix) == \
            f"{prefix}: march_sh is forward-only (call under torch.no_grad(); {REASON})"


def test_literals():
    """The strings as a caller sees them, written out."""
    check = sparse_field.check_march_sh
    assert refusal(check, "ray", GRID, "render") == "render: march_sh must be None, 'rows' or 'rays', got 'ray'"
    assert refusal(check, "rays", None, "render_rays") == \
        "render_rays: march_sh='rays' needs march= (the ray index belongs to a grid march's list)"
    with torch.enable_grad():
        assert refusal(check, "rays", GRID, "render_rays") == \
            ("render_rays: march_sh is forward-only (call under torch.no_grad(); the backward reads per-point SH "
             "rows)")


def test_render_rays_and_render_refuse_before_anything_else():
    """Both entry points run the check on their own keywords before they touch the rays: the refusals fire with
    arguments that could not render anything."""
    import indoor_nerf_amd as nerf
    _, net, _, _ = field_modules()
    common = dict(network_fn=net, network_query_fn=None, N_samples=4)
    with torch.no_grad():
        assert refusal(nerf.render_rays, None, march_sh="rays", **common) == f"render_rays: {NEEDS_MARCH}"
        assert refusal(nerf.render_rays, None, march_sh="points", march=GRID, **common) == \
            "render_rays: march_sh must be None, 'rows' or 'rays', got 'points'"
        assert refusal(nerf.render, 2, 2, None, march_sh="rays", **common) == f"render: {NEEDS_MARCH}"
        assert refusal(nerf.render, 2, 2, None, march_sh=3, march=GRID, **common) == \
            "render: march_sh must be None, 'rows' or 'rays', got 3"
    with torch.enable_grad():
        for fn, args, prefix in ((nerf.render_rays, (None,), "render_rays"), (nerf.render, (2, 2, None), "render")):
            assert refusal(fn, *args, march_sh="rays", march=GRID, **common) == \
                f"{prefix}: march_sh is forward-only (call under torch.no_grad(); {REASON})"


def test_request_carries_either_the_rows_or_the_index():
    """No global switch and no further attribute on the points: the request's MarchList holds sh_c, or ray_c and
    sh_rec (`used` is the request's)."""
    Req = sparse_field.MarchList
    sh_c, ray_c, rec = torch.zeros(5, 16), torch.zeros(5, dtype=torch.int32), torch.zeros(2, 40)
    a = Req(sh_c, 1000)
    assert a.sh_c is sh_c and a.ray_c is None and a.sh_rec is None and a.max_points == 1000
    assert sparse_field.FieldRequest(march=a).used is False
    b = Req(None, 1000, ray_c=ray_c, sh_rec=rec)
    assert b.sh_c is None and b.ray_c is ray_c and b.sh_rec is rec and sparse_field.FieldRequest(march=b).what == "march"
    for args, kw in (((None,), {}), ((sh_c,), dict(ray_c=ray_c, sh_rec=rec)), ((None,), dict(ray_c=ray_c)),
                     ((None,), dict(sh_rec=rec)), ((sh_c,), dict(sh_rec=rec))):
        assert refusal(Req, *args, **kw) == "march: a request carries either sh_c or (ray_c, sh_rec)"
    assert sorted(k for k in vars(b)) == ["max_points", "ray_c", "sh_c", "sh_rec"]


def test_mlp_forward_chooses_the_entry(monkeypatch):
    """sparse_field.mlp_forward is the one place that picks the entry: by the request's bf16 and packed (not by there
    being a request: one with only half=True runs the fp32-accurate entries), and by whether the call brings a ray
    index."""
    import indoor_nerf_amd._lib as L
    seen = []
    monkeypatch.setattr(L, "call", lambda name, *args: seen.append((name, args)))
    monkeypatch.setattr(L, "stream", lambda: "stream")
    Req = sparse_field.FieldRequest
    for mlp, rows_entry, rays_entry, stride in ((None, "nerf_mlp_fwd_ord", "nerf_mlp_fwd_rays", 2),
                                                (Req(bf16=True), "nerf_mlp_fwd_bf16", "nerf_mlp_fwd_bf16_rays", 2),
                                                (Req(bf16=True, packed=True), "nerf_mlp_fwd_bf16_pkbf",
                                                 "nerf_mlp_fwd_bf16_pkbf_rays", 1),
                                                (Req(half=True), "nerf_mlp_fwd_ord", "nerf_mlp_fwd_rays", 2)):
        sparse_field.mlp_forward(mlp, "feat", 77, "sh_c", "keep", 9, "w", "raw", None)
        assert seen[-1][0] == rows_entry and seen[-1][1][:7] == ("feat", stride, 77, "sh_c", 16, None, 1)
        sparse_field.mlp_forward(mlp, "feat", 77, None, "keep", 9, "w", "raw", None, ("ray_of", "rec", 4))
        assert seen[-1] == (rays_entry, ("feat", stride, 77, "rec", "ray_of", 4, "keep", 9, "w", "raw", "stream"))
        n = len(seen)
        for sh_c, order in (("sh_c", None), (None, "order")):
            assert refusal(sparse_field.mlp_forward, mlp, "feat", 77, sh_c, "keep", 9, "w", "raw", order,
                           ("ray_of", "rec", 4)) == "march_sh: a ray index replaces the SH rows and has no point order"
        assert len(seen) == n
