"""CPU-only: the one request that carries every forward-only keyword from render_rays to the fused run_network
(sparse_field.FieldOptions / FieldRequest, render._query). Nothing here needs a device or the built
library: render_rays is run up to its first field call with the launches stubbed out."""
import pytest
import torch

from indoor_nerf_amd import sparse_field

from test_forward_only_guards import field_modules, refusal

GRID = object()      # the checks below only ask whether a grid was given
KEYWORDS = ("march", "march_sh", "march_stop", "march_stop_slab", "mlp_precision", "table_precision",
            "feature_precision")
NONE = dict(march=None, march_sh=None, march_stop=None, march_stop_slab=128, mlp_precision=None, table_precision=None,
            feature_precision=None)
# one bad keyword each (the guard modules' lists), with the checker that refuses it on its own
BAD = [(dict(march_sh=v, march=m), lambda p, v=v, m=m: sparse_field.check_march_sh(v, m, p))
       for v, m in [("ray", None), ("RAYS", GRID), ("", GRID), (1, None), (True, GRID), (b"rays", GRID), ("rays", None)]]
BAD += [(dict(march_stop=v, march_stop_slab=s, march=m), lambda p, v=v, s=s, m=m: sparse_field.check_march_stop(v, s, m, p))
        for v, s, m in [(1e-2, 128, None), (0, 128, GRID), (1.0, 128, GRID), (True, 128, GRID), ("1e-2", 128, GRID),
                        (1e-2, 0, GRID), (1e-2, 2.5, GRID), (1e-2, True, GRID)]]
BAD += [(dict(mlp_precision=v), lambda p, v=v: sparse_field.check_mlp_precision(v, p))
        for v in ("fp16", "BF16", "", 16, True, 0.5, b"bf16", ("bf16",))]
BAD += [(dict(feature_precision=v, mlp_precision=m), lambda p, v=v, m=m: sparse_field.check_feature_precision(v, m == "bf16", p))
        for v, m in [("fp16", "bf16"), ("BF16", None), (16, "bf16"), (True, None), (torch.bfloat16, "bf16"),
                     ("bf16", None), ("bf16", "fp32")]]
BAD += [(dict(table_precision=v), lambda p, v=v: sparse_field.check_table_precision(v, p))
        for v in ("bf16", "FP16", "half", "", 16, True, 0.5, b"fp16", ("fp16",), torch.float16)]


def options(prefix, **kw):
    return sparse_field.field_options(prefix, **dict(NONE, **kw))


# ---------------------------------------------------------------- the two types
def test_request_refusals_and_properties():
    Req, march = sparse_field.FieldRequest, sparse_field.MarchList(torch.zeros(3, 16))
    assert refusal(Req, packed=True) == "field request: packed bf16 features need the bf16 MLP"
    assert refusal(Req, half=True, packed=True) == "field request: packed bf16 features need the bf16 MLP"
    for kw in (dict(grid=GRID), dict(early=(None, None, 1e-3, 8)), dict(grid=GRID, early=(None, None, 1e-3, 8))):
        assert refusal(Req, march=march, **kw) == \
            "field request: a march's list does not combine with a grid or early termination"
    early = (None, None, 1e-3, 8)
    shapes = [(dict(), None), (dict(grid=GRID), "occupancy"), (dict(early=early), "early_stop"),
              (dict(grid=GRID, early=early), "early_stop"), (dict(march=march), "march")]
    for kw, what in shapes:
        for bf16, half, packed in ((False, False, False), (True, False, False), (True, False, True),
                                   (False, True, False), (True, True, False), (True, True, True)):
            req = Req(bf16=bf16, half=half, packed=packed, **kw)
            assert req.what == what
            assert req.blame == ("table_precision" if half else "mlp_precision" if bf16 else what)
            assert (req.bf16, req.half, req.packed) == (bf16, half, packed)
            assert req.used is False and req.stop is None
    assert sorted(vars(Req())) == ["bf16", "early", "grid", "half", "march", "packed", "stop", "used"]


def test_options_are_immutable_and_build_the_request():
    with torch.no_grad():
        opts = options("render", march=GRID, march_sh="rays", march_stop=1e-2, march_stop_slab=8, mlp_precision="bf16",
                       table_precision="fp16", feature_precision="bf16")
        assert opts == sparse_field.FieldOptions(bf16=True, half=True, packed=True, by_ray=True, stop=(1e-2, 8))
        assert options("render") == sparse_field.FieldOptions() == (False, False, False, False, None)
        assert options("render", mlp_precision="fp32", table_precision="fp32", feature_precision="fp32",
                       march_sh="rows") == sparse_field.FieldOptions()
    with pytest.raises(AttributeError):
        opts.bf16 = False
    # nothing asked: no request at all; anything asked: one request with the call's flags
    assert sparse_field.FieldOptions().request() is None
    assert sparse_field.FieldOptions(by_ray=True, stop=(1e-2, 8)).request() is None
    req = opts.request(grid=GRID)
    assert (req.grid, req.early, req.march, req.bf16, req.half, req.packed) == (GRID, None, None, True, True, True)
    assert sparse_field.FieldOptions().request(early=(None, None, 1e-3, 8)).what == "early_stop"
    assert sparse_field.FieldOptions(half=True).request().blame == "table_precision"
    a, b = opts.request(), opts.request()
    assert a is not b      # `used` and `stop` belong to one field call


# ---------------------------------------------------------------- one check for both entry points
@pytest.mark.parametrize("case", range(len(BAD)))
def test_field_options_gives_each_checkers_refusal_under_both_prefixes(case):
    kw, alone = BAD[case]
    with torch.no_grad():
        words = {}
        for prefix in ("render_rays", "render"):
            words[prefix] = refusal(options, prefix, **kw)
            assert words[prefix] == refusal(alone, prefix) and words[prefix].startswith(prefix + ": ")
        assert words["render"] == "render" + words["render_rays"][len("render_rays"):]


def test_gradients_are_refused_in_one_order():
    """The checkers run in one fixed order: march_sh, march_stop, mlp_precision, feature_precision, table_precision."""
    by_ray, bf16, tab = dict(march_sh="rays", march=GRID), dict(mlp_precision="bf16"), dict(table_precision="fp16")
    for prefix in ("render_rays", "render"):
        with torch.enable_grad():       # with gradients every forward-only keyword refuses: the first one wins
            for first, both in (("march_sh", dict(by_ray, **bf16)), ("march_sh", dict(by_ray, **tab)),
                                ("mlp_precision", dict(bf16, feature_precision="bf16")),
                                ("mlp_precision", dict(bf16, **tab)),
                                ("march_sh", dict(by_ray, feature_precision="bf16", **bf16, **tab))):
                assert refusal(options, prefix, **both).startswith(f"{prefix}: {first} is forward-only")
            # a bad value before a later keyword's gradients
            assert refusal(options, prefix, mlp_precision="half", **tab) == \
                f"{prefix}: mlp_precision must be None, 'fp32' or 'bf16', got 'half'"
        with torch.no_grad():
            assert refusal(options, prefix, march_stop=1e-2, mlp_precision="half") == \
                f"{prefix}: march_stop needs march= (rays are stopped inside a grid march; early_stop= is the dense path's)"
            assert refusal(options, prefix, march_sh="ray", march_stop=1e-2) == \
                f"{prefix}: march_sh must be None, 'rows' or 'rays', got 'ray'"
            assert refusal(options, prefix, feature_precision="half", table_precision="half", **bf16) == \
                f"{prefix}: feature_precision must be None, 'fp32' or 'bf16', got 'half'"


def test_render_rays_and_render_both_go_through_field_options(monkeypatch):
    import indoor_nerf_amd as nerf
    calls, real = [], sparse_field.field_options

    def recording(*args, **kwargs):
        calls.append((args, kwargs))
        return real(*args, **kwargs)
    monkeypatch.setattr(sparse_field, "field_options", recording)
    _, net, _, _ = field_modules()
    common = dict(network_fn=net, network_query_fn=None, N_samples=4)
    asked = dict(feature_precision="bf16", mlp_precision="fp32", table_precision="fp16", march=GRID, march_sh="rows",
                 march_stop=0.5, march_stop_slab=7)
    with torch.no_grad():
        assert refusal(nerf.render_rays, None, **asked, **common).startswith("render_rays: feature_precision='bf16' needs")
        assert refusal(nerf.render, 2, 2, None, **asked, **common).startswith("render: feature_precision='bf16' needs")
    assert [(a, k) for a, k in calls] == [
        (("render_rays", GRID, "rows", 0.5, 7, "fp32", "fp16", "bf16"), {}),
        (("render", GRID, "rows", 0.5, 7, "fp32", "fp16", "bf16"), {})]
    # and with no keyword at all: the defaults, nothing else
    del calls[:]
    monkeypatch.setattr(sparse_field, "field_options", lambda *a: calls.append(a) or (_ for _ in ()).throw(ValueError("seen")))
    assert refusal(nerf.render_rays, None, **common) == "seen" and refusal(nerf.render, 2, 2, None, **common) == "seen"
    assert calls == [("render_rays", None, None, None, 128, None, None, None),
                     ("render", None, None, None, 128, None, None, None)]


# ---------------------------------------------------------------- one attribute, one wrapper
class Boom(Exception):
    pass


def request_shapes():
    z, rays_d = torch.zeros(2, 3), torch.zeros(2, 3)
    return {"occupancy": dict(grid=GRID), "early_stop": dict(early=(z, rays_d, 1e-3, 8)),
            "occupancy + early_stop": dict(grid=GRID, early=(z, rays_d, 1e-3, 8)),
            "march": dict(march=sparse_field.MarchList(torch.zeros(6, 16))),
            "march by ray": dict(march=sparse_field.MarchList(None, ray_c=torch.zeros(6, dtype=torch.int32),
                                                              sh_rec=torch.zeros(2, 40)))}


@pytest.mark.parametrize("shape", list(request_shapes()))
@pytest.mark.parametrize("precisions", [dict(), dict(bf16=True, half=True, packed=True)])
def test_an_exception_in_the_query_function_leaves_nothing_on_the_points(shape, precisions):
    from indoor_nerf_amd.render import _query
    pts, seen = torch.zeros(2, 3, 3), []

    def failing(p, viewdirs, fn):
        seen.append(sorted(k for k in vars(p) if k.startswith("_nerf")))
        raise Boom()

    req = sparse_field.FieldRequest(**request_shapes()[shape], **precisions)
    with pytest.raises(Boom):
        _query(failing, pts, None, None, req)
    assert seen == [["_nerf_req"]]
    assert not any(k.startswith("_nerf") for k in vars(pts))
    assert req.used is False


def stub_launches(monkeypatch):
    import indoor_nerf_amd._lib as L
    monkeypatch.setattr(L, "call", lambda name, *args: None)
    monkeypatch.setattr(L, "ptr", lambda *args, **kwargs: None)
    monkeypatch.setattr(L, "stream", lambda: None)


@pytest.mark.parametrize("over", [dict(occupancy=GRID), dict(early_stop=1e-3, early_stop_slab=8),
                                  dict(occupancy=GRID, early_stop=1e-3, mlp_precision="bf16", table_precision="fp16")])
def test_render_rays_leaves_nothing_on_its_points_when_the_query_function_raises(monkeypatch, over):
    import indoor_nerf_amd as nerf
    stub_launches(monkeypatch)
    _, net, _, _ = field_modules()
    held = []

    def failing(p, viewdirs, fn):
        held.append((p, p._nerf_req))
        raise Boom()

    with torch.no_grad(), pytest.raises(Boom):
        nerf.render_rays(torch.zeros(4, 11), net, failing, N_samples=3, **over)
    (pts, req), = held
    assert req.what == ("occupancy" if "early_stop" not in over else "early_stop")
    assert (req.bf16, req.half) == ("mlp_precision" in over, "table_precision" in over)
    assert tuple(pts.shape) == (4, 3, 3) and not any(k.startswith("_nerf") for k in vars(pts))


def test_render_rays_without_a_forward_only_keyword_attaches_nothing(monkeypatch):
    import indoor_nerf_amd as nerf
    stub_launches(monkeypatch)

    def no_request(*args, **kwargs):
        raise AssertionError("a plain render_rays call built a FieldRequest")
    monkeypatch.setattr(sparse_field, "FieldRequest", no_request)
    _, net, _, _ = field_modules()
    seen = []

    def plain(p, viewdirs, fn):
        seen.append(sorted(k for k in vars(p) if k.startswith("_nerf")))
        raise Boom()

    for grad in (torch.no_grad, torch.enable_grad):
        for kw in (dict(), dict(mlp_precision="fp32", table_precision="fp32", feature_precision="fp32", march_sh="rows")):
            with grad(), pytest.raises(Boom):
                nerf.render_rays(torch.zeros(4, 11), net, plain, N_samples=3, **kw)
            assert seen[-1] == []      # no coarse-feature reuse either: N_importance is 0
            with grad(), pytest.raises(Boom):
                nerf.render_rays(torch.zeros(4, 11), net, plain, N_samples=3, N_importance=2, network_fine=net, **kw)
            assert seen[-1] == ["_nerf_reuse"]
