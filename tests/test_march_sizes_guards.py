"""CPU-only: the refusals of march_sizes= (launches sized on the device in the grid march), word for
word, the order they come in, and the request that carries the device total. The checkers are called directly, as in
test_march_sh_guards.py: nothing here needs a device or the built library, and every refusal below is raised before
anything could be launched."""
import pytest
import torch

from indoor_nerf_amd import sparse_field

from test_forward_only_guards import field_modules, refusal

REASON = "the backward needs the list lengths on the host"
NEEDS_MARCH = "march_sizes='device' needs march= (the sizes are those of a grid march's lists)"
NEEDS_RAYS = "march_sizes='device' needs march_sh='rays' (the device-sized MLP reads SH through the ray index)"
NEEDS_MLP = "march_sizes='device' needs mlp_precision='bf16' (the device-sized MLP is the bf16 forward)"
NEEDS_FEAT = ("march_sizes='device' needs feature_precision='bf16' (the device-sized encoder writes packed bf16 "
              "features)")
GRID = object()      # the value checks only ask whether march= was given
FAST = dict(march_sh="rays", mlp_precision="bf16", feature_precision="bf16")


def test_reason_is_listed():
    assert sparse_field.NOT_IN_TRAINING["march_sizes"] == REASON
    assert sparse_field.NOT_IN_TRAINING["march_sh"] == "the backward reads per-point SH rows"      # the others keep theirs
    assert sparse_field.NOT_IN_TRAINING["march"] == "rays are not marched in training"


@pytest.mark.parametrize("prefix", ["render_rays", "render"])
def test_value_companions_and_gradients(prefix):
    check = sparse_field.check_march_sizes
    for grad in (torch.no_grad, torch.enable_grad):
        with grad():
            for march in (None, GRID):
                for flags in ((False, False, False), (True, True, True)):
                    # today's path: nothing to refuse, with or without gradients, a march or the companions
                    assert check(None, march, *flags, prefix) is False and check("host", march, *flags, prefix) is False
                    for bad in ("dev", "DEVICE", "gpu", "", 1, True, 0.5, b"device", ("device",), torch.int32):
                        assert refusal(check, bad, march, *flags, prefix) == \
                            f"{prefix}: march_sizes must be None, 'host' or 'device', got {bad!r}"
            # the march, then the three companions in this order, all before the gradients
            assert refusal(check, "device", None, True, True, True, prefix) == f"{prefix}: {NEEDS_MARCH}"
            assert refusal(check, "device", GRID, False, False, False, prefix) == f"{prefix}: {NEEDS_RAYS}"
            assert refusal(check, "device", GRID, True, False, False, prefix) == f"{prefix}: {NEEDS_MLP}"
            assert refusal(check, "device", GRID, True, True, False, prefix) == f"{prefix}: {NEEDS_FEAT}"
            assert refusal(check, "device", GRID, False, True, True, prefix) == f"{prefix}: {NEEDS_RAYS}"
    with torch.no_grad():
        assert check("device", GRID, True, True, True, prefix) is True
    with torch.enable_grad():
        assert refusal(check, "device", GRID, True, True, True, prefix) == \
            f"{prefix}: march_sizes is forward-only (call under torch.no_grad(); {REASON})"


def test_literals():
    """The strings as a caller sees them, written out."""
    check = sparse_field.check_march_sizes
    assert refusal(check, "gpu", GRID, True, True, True, "render") == \
        "render: march_sizes must be None, 'host' or 'device', got 'gpu'"
    assert refusal(check, "device", None, True, True, True, "render_rays") == \
        "render_rays: march_sizes='device' needs march= (the sizes are those of a grid march's lists)"
    assert refusal(check, "device", GRID, False, True, True, "render") == \
        "render: march_sizes='device' needs march_sh='rays' (the device-sized MLP reads SH through the ray index)"
    assert refusal(check, "device", GRID, True, False, True, "render") == \
        "render: march_sizes='device' needs mlp_precision='bf16' (the device-sized MLP is the bf16 forward)"
    assert refusal(check, "device", GRID, True, True, False, "render_rays") == \
        ("render_rays: march_sizes='device' needs feature_precision='bf16' (the device-sized encoder writes packed "
         "bf16 features)")
    with torch.enable_grad():
        assert refusal(check, "device", GRID, True, True, True, "render_rays") == \
            ("render_rays: march_sizes is forward-only (call under torch.no_grad(); the backward needs the list "
             "lengths on the host)")


@pytest.mark.parametrize("prefix", ["render_rays", "render"])
def test_field_options_checks_it_last_and_leaves_it_out(prefix):
    options = sparse_field.field_options
    base = (prefix, GRID, "rays", None, 128, "bf16", None, "bf16")
    with torch.no_grad():
        opts = options(*base, march_sizes="device")
        assert opts == options(*base) == sparse_field.FieldOptions(True, False, True, True, None)
        assert options(*base, "host") == opts and options(*base, None) == opts
        assert sparse_field.device_sized("device") is True
        assert not any(sparse_field.device_sized(v) for v in (None, "host", "dev", 1, True))
        # an earlier keyword's refusal comes first
        assert refusal(options, prefix, GRID, "ray", None, 128, "bf16", None, "bf16", march_sizes="device") == \
            f"{prefix}: march_sh must be None, 'rows' or 'rays', got 'ray'"
        assert refusal(options, prefix, GRID, "rays", None, 128, "bf16", "fp8", "bf16", march_sizes="device") == \
            f"{prefix}: table_precision must be None, 'fp32' or 'fp16', got 'fp8'"
        assert refusal(options, prefix, GRID, "rays", None, 128, "bf16", None, "bf16", march_sizes="gpu") == \
            f"{prefix}: march_sizes must be None, 'host' or 'device', got 'gpu'"
        assert refusal(options, prefix, GRID, "rays", None, 128, "bf16", None, None, march_sizes="device") == \
            f"{prefix}: {NEEDS_FEAT}"
        assert refusal(options, prefix, GRID, "rays", None, 128, None, None, None, march_sizes="device") == \
            f"{prefix}: {NEEDS_MLP}"
        assert refusal(options, prefix, GRID, None, None, 128, "bf16", None, "bf16", march_sizes="device") == \
            f"{prefix}: {NEEDS_RAYS}"
        assert refusal(options, prefix, None, None, None, 128, "bf16", None, "bf16", march_sizes="device") == \
            f"{prefix}: {NEEDS_MARCH}"
        # it composes with march_stop and the fp16 tables
        assert options(prefix, GRID, "rays", 1e-3, 8, "bf16", "fp16", "bf16", march_sizes="device") == \
            sparse_field.FieldOptions(True, True, True, True, (1e-3, 8))


def test_render_rays_and_render_refuse_before_anything_else():
    """Both entry points run the check on their own keywords before they touch the rays: the refusals fire with
    arguments that could not render anything."""
    import indoor_nerf_amd as nerf
    _, net, _, _ = field_modules()
    common = dict(network_fn=net, network_query_fn=None, N_samples=4)
    with torch.no_grad():
        for fn, args, prefix in ((nerf.render_rays, (None,), "render_rays"), (nerf.render, (2, 2, None), "render")):
            assert refusal(fn, *args, march_sizes="device", **common) == f"{prefix}: {NEEDS_MARCH}"
            assert refusal(fn, *args, march_sizes="device", march=GRID, **common) == f"{prefix}: {NEEDS_RAYS}"
            assert refusal(fn, *args, march_sizes="device", march=GRID, march_sh="rays", **common) == \
                f"{prefix}: {NEEDS_MLP}"
            assert refusal(fn, *args, march_sizes="device", march=GRID, march_sh="rays", mlp_precision="bf16",
                           **common) == f"{prefix}: {NEEDS_FEAT}"
            assert refusal(fn, *args, march_sizes="sizes", march=GRID, **FAST, **common) == \
                f"{prefix}: march_sizes must be None, 'host' or 'device', got 'sizes'"
    with torch.enable_grad():       # the companions are forward-only themselves and are checked first
        for fn, args, prefix in ((nerf.render_rays, (None,), "render_rays"), (nerf.render, (2, 2, None), "render")):
            assert refusal(fn, *args, march_sizes="device", march=GRID, **FAST, **common) == \
                f"{prefix}: march_sh is forward-only (call under torch.no_grad(); the backward reads per-point SH rows)"


def test_list_carries_the_total_and_the_capacity():
    Req = sparse_field.MarchList
    ray_c, rec, total = torch.zeros(5, dtype=torch.int32), torch.zeros(2, 40), torch.zeros(1, dtype=torch.int32)
    a = Req(None, 1000, ray_c=ray_c, sh_rec=rec)
    assert a.total is None and a.capacity is None
    assert sorted(vars(a)) == ["max_points", "ray_c", "sh_c", "sh_rec"]      # a host-sized list is what it was
    b = Req(None, 1000, ray_c=ray_c, sh_rec=rec, total=total, capacity=5)
    assert b.total is total and b.capacity == 5 and b.ray_c is ray_c and b.sh_rec is rec
    assert sparse_field.FieldRequest(march=b, bf16=True, packed=True).what == "march"
    msg = "march: a device-sized list carries (total, capacity) and a ray index"
    assert refusal(Req, None, 1000, ray_c=ray_c, sh_rec=rec, total=total) == msg
    assert refusal(Req, None, 1000, ray_c=ray_c, sh_rec=rec, capacity=5) == msg
    assert refusal(Req, torch.zeros(5, 16), 1000, total=total, capacity=5) == msg


def test_device_sized_field_call_refuses_other_precisions():
    """run_network_packed with a device total and a request that is not the bf16 MLP on packed features: refused
    before any launch (render_rays never builds such a request: check_march_sizes refuses first)."""
    emb, net, _, sh = field_modules()
    ray_c, rec, total = torch.zeros(5, dtype=torch.int32), torch.zeros(2, 40), torch.zeros(1, dtype=torch.int32)
    march = sparse_field.MarchList(None, 1000, ray_c=ray_c, sh_rec=rec, total=total, capacity=5)
    pts, dirs = torch.zeros(5, 3), torch.zeros(2, 3)
    with torch.no_grad():
        for kw in ({}, dict(bf16=True), dict(half=True)):
            req = sparse_field.FieldRequest(march=march, **kw)
            assert refusal(sparse_field.run_network_packed, pts, dirs, net, emb, sh, req) == \
                "march: a device-sized list needs the bf16 MLP on packed bf16 features"
        req = sparse_field.FieldRequest(march=march, bf16=True, packed=True)
        assert refusal(sparse_field.run_network_packed, pts[:4], dirs, net, emb, sh, req) == \
            "march: ray index / SH records / total of the request do not match the points"
    with torch.enable_grad():
        assert refusal(sparse_field.run_network_packed, pts, dirs, net, emb, sh, req) == \
            "march: forward-only (call under torch.no_grad(); rays are not marched in training)"
