"""render_rays(mlp_precision="bf16", feature_precision="bf16"), needs an MI355X: every hash-encoding
launch of a forward-only render writes packed bf16 words (nerf_hash_encode_fwd_pkbf, with fp16 tables
nerf_hash_encode_fwd_half_pkbf) and every MLP forward launch reads them (nerf_mlp_fwd_bf16_pkbf), on the dense path
and on every path that skips samples; None and "fp32" are the call without the keyword, bit for bit.

The specification needs no tolerance: the encoder does the rounding the bf16 MLP does first (test_gpu_feat_bf16.py),
so a frame with the keyword must equal, in every entry and every bit, the frame with mlp_precision="bf16" alone. The
routing test is what keeps that equality from being met by a keyword that is ignored.

The scene of forward_only.py (build_scene) with the sigma row of both networks scaled by 500, as
test_gpu_render_fp16_tables.py uses it.
"""
import pytest
import torch

from forward_only import H, W, ball_mask, bits_equal, build_scene
from test_gpu_march import march_rays
from test_gpu_render_fp16_tables import MASKS, PACKED, SIGMA_SCALE, VARIANTS, assert_same, same_bits, variants

pytestmark = pytest.mark.gpu

ENC = {None: "nerf_hash_encode_fwd_q", "fp16": "nerf_hash_encode_fwd_half"}     # the entries the package calls
ENC_PK = {None: "nerf_hash_encode_fwd_pkbf", "fp16": "nerf_hash_encode_fwd_half_pkbf"}
MLP, MLP_PK = "nerf_mlp_fwd_bf16", "nerf_mlp_fwd_bf16_pkbf"
BF16 = dict(mlp_precision="bf16")
PACKED_KW = dict(mlp_precision="bf16", feature_precision="bf16")
STOP = "march+march_stop"
ALL = VARIANTS + [STOP]


@pytest.fixture(scope="module")
def scene(nerf, gpu):
    return build_scene(nerf, gpu, SIGMA_SCALE)


def variant(scene, name):
    if name == STOP:
        return dict(march=scene["grid_of"](ball_mask()), march_samples=64, march_stop=0.9, march_stop_slab=8,
                    retraw=False)
    return variants(scene)[name]


def tables(tab):
    return {} if tab is None else dict(table_precision=tab)


# ---------------------------------------------------------------- 1. the frame is the bf16 frame
@pytest.mark.parametrize("tab", [None, "fp16"])
@pytest.mark.parametrize("name", ALL)
def test_frame_equals_the_bf16_frame(nerf, gpu, scene, name, tab):
    for i in (0, 1):
        got = scene["frame"](i, **variant(scene, name), **tables(tab), **PACKED_KW)
        ref = scene["frame"](i, **variant(scene, name), **tables(tab), **BF16)
        assert_same(got, ref, f"{name} pose {i} tables {tab}")
        if name == STOP:
            assert bool((ref["march_stop_samples"] < 64).any()), "fixture: no ray stops"


# ---------------------------------------------------------------- 2. the packed entries of a march
@pytest.mark.parametrize("tab", [None, "fp16"])
@pytest.mark.parametrize("which,K", [("ball16", 64), ("random5", 200)])
def test_march_packed_entries(nerf, gpu, scene, which, K, tab):
    for i in (0, 1):
        got = march_rays(nerf, scene, i, scene["grid_of"](MASKS[which]()), K, **tables(tab), **PACKED_KW)
        ref = march_rays(nerf, scene, i, scene["grid_of"](MASKS[which]()), K, **tables(tab), **BF16)
        assert ref["raw"].shape[0] > 0
        for k in PACKED:
            assert same_bits(got[k], ref[k]), f"{which} K {K} pose {i} tables {tab}: {k}"


@pytest.mark.parametrize("tab", [None, "fp16"])
def test_march_stop_slabs(nerf, gpu, scene, tab):
    """With march_stop the packed entries come per slab: every tuple of march_slabs is the same bits."""
    for i in (0, 1):
        kw = dict(march_stop=0.9, march_stop_slab=8, **tables(tab))
        got = march_rays(nerf, scene, i, scene["grid_of"](ball_mask()), 64, **kw, **PACKED_KW)
        ref = march_rays(nerf, scene, i, scene["grid_of"](ball_mask()), 64, **kw, **BF16)
        assert len(got["march_slabs"]) == len(ref["march_slabs"]) == 8
        assert sum(s[1].shape[0] for s in ref["march_slabs"]) > 0
        for n, (a, b) in enumerate(zip(got["march_slabs"], ref["march_slabs"])):
            for x, y, k in zip(a, b, ("offsets", "raw", "pts", "z_vals")):
                assert same_bits(x, y), f"pose {i} tables {tab} slab {n}: {k}"
        for k in ("rgb_map", "depth_map", "acc_map", "march_samples", "march_stop_samples"):
            assert same_bits(got[k], ref[k]), f"pose {i} tables {tab}: {k}"


# ---------------------------------------------------------------- 3. routing
def calls(scene, monkeypatch, i, **over):
    """(frame i, the names of its hash-encoding forward launches, of its MLP forward launches). The query function is
    named, so that build_scene's frame cache is not used: a cached frame launches nothing."""
    import indoor_nerf_amd._lib as L
    names, call = [], L.call

    def recording(name, *args):
        names.append(name)
        return call(name, *args)
    over.setdefault("network_query_fn", scene["kw"]["network_query_fn"])
    with monkeypatch.context() as m:
        m.setattr(L, "call", recording)
        out = scene["frame"](i, **over)
    return (out, [n for n in names if n.startswith("nerf_hash_encode_fwd")],
            [n for n in names if n.startswith("nerf_mlp_fwd")])


@pytest.mark.parametrize("tab", [None, "fp16"])
@pytest.mark.parametrize("name", ALL)
def test_routing(nerf, gpu, scene, name, tab, monkeypatch):
    over = dict(variant(scene, name), **tables(tab))
    base, enc, mlp = calls(scene, monkeypatch, 0, **over, **BF16)
    assert enc and mlp and enc == [ENC[tab]] * len(enc) and mlp == [MLP] * len(mlp), f"{name}: {enc} {mlp}"
    for value in (None, "fp32"):
        same, enc2, mlp2 = calls(scene, monkeypatch, 0, feature_precision=value, **over, **BF16)
        assert (enc2, mlp2) == (enc, mlp), f"{name} feature_precision={value!r}: {enc2} {mlp2}"
        assert_same(same, base, f"{name} feature_precision={value!r}")
    got, enc3, mlp3 = calls(scene, monkeypatch, 0, **over, **PACKED_KW)
    assert enc3 == [ENC_PK[tab]] * len(enc) and mlp3 == [MLP_PK] * len(mlp), f"{name} packed: {enc3} {mlp3}"
    assert_same(got, base, f"{name} packed")
    # without mlp_precision the keyword's None / "fp32" reach the fp32-accurate MLP as before
    plain, enc4, mlp4 = calls(scene, monkeypatch, 0, feature_precision="fp32", **over)
    assert enc4 == enc and len(mlp4) == len(mlp) and not any("bf16" in n for n in mlp4), f"{name}: {mlp4}"
    assert not bits_equal(plain["rgb_map"], base["rgb_map"]), f"{name}: the bf16 frame has the fp32 frame's bits"


# ---------------------------------------------------------------- 4. coarse-feature reuse
@pytest.mark.parametrize("tab", [None, "fp16"])
def test_fine_pass_with_and_without_coarse_reuse(nerf, gpu, scene, tab, monkeypatch):
    """The dense fine pass in both forms: the importance samples alone gathered into the head rows of the packed
    reuse buffer (the MLP walks the importance-first order over words), and every point re-encoded."""
    import importlib
    R = importlib.import_module("indoor_nerf_amd.render")
    with_reuse, enc, mlp = calls(scene, monkeypatch, 1, **tables(tab), **PACKED_KW)
    assert enc == [ENC_PK[tab]] * 2 and mlp == [MLP_PK] * 2 and R.last_reuse_used()
    R.set_coarse_reuse(False)
    try:
        without, enc, mlp = calls(scene, monkeypatch, 1, **tables(tab), **PACKED_KW)
        assert enc == [ENC_PK[tab]] * 2 and mlp == [MLP_PK] * 2 and not R.last_reuse_used()
    finally:
        R.set_coarse_reuse(True)
    assert_same(with_reuse, without, "coarse reuse on / off")
    assert_same(with_reuse, scene["frame"](1, **tables(tab), **BF16), "against the bf16 frame")


# ---------------------------------------------------------------- 5. chunking
@pytest.mark.parametrize("name", ["dense", "occupancy+early_stop", "march K 64", STOP])
def test_chunks_give_the_same_bits(nerf, gpu, scene, name):
    """Chunks of 37 rays (odd feature buffers, tail lanes in every launch) and one chunk of 4096."""
    for i in (0, 1):
        small = scene["frame"](i, chunk=37, **variant(scene, name), **PACKED_KW)
        whole = scene["frame"](i, chunk=4096, **variant(scene, name), **PACKED_KW)
        assert_same(small, whole, f"{name} pose {i}: chunks of 37 and of 4096 rays")
        assert_same(small, scene["frame"](i, chunk=37, **variant(scene, name), **BF16), f"{name} pose {i}: chunk 37")


# ---------------------------------------------------------------- 6. refusals, through render_rays / render
def test_refusals(nerf, gpu, scene):
    kw, frame = scene["kw"], scene["frame"]
    nqf = kw["network_query_fn"]
    needs = "feature_precision='bf16' needs mlp_precision='bf16' \\(the fp32-accurate MLP reads fp32 features\\)"

    def run(**over):
        return frame(0, **dict(dict(PACKED_KW, network_query_fn=nqf), **over))

    def rays(**over):
        return nerf.render_rays(scene["packed"](0), **scene["ray_kw"](**dict(PACKED_KW, **over)))

    run()                                                                   # the supported call
    run(raw_noise_std=1.0)                                                  # noise is added after the field
    with pytest.raises(ValueError, match="render: feature_precision must be None, 'fp32' or 'bf16', got 'fp16'"):
        run(feature_precision="fp16")
    with torch.no_grad(), pytest.raises(ValueError, match="render_rays: feature_precision must be None, 'fp32' or 'bf16'"):
        rays(feature_precision=16)
    for mlp in (None, "fp32"):
        with pytest.raises(ValueError, match="render: " + needs):
            run(mlp_precision=mlp)
        with torch.no_grad(), pytest.raises(ValueError, match="render_rays: " + needs):
            rays(mlp_precision=mlp)
    with torch.enable_grad(), pytest.raises(ValueError, match="render: mlp_precision is forward-only"):
        nerf.render(H, W, scene["K"], c2w=scene["poses"][0][:3, :4].to(gpu), **dict(kw, **PACKED_KW))
    with torch.enable_grad(), pytest.raises(ValueError, match="render_rays: mlp_precision is forward-only"):
        rays()
    # the MLP's module refusals hold: a normals head, A-CAQ quantizers
    head = nerf.NeRFSmall(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64,
                          input_ch=32, input_ch_views=16, predict_normals=True).to(gpu).eval()
    with pytest.raises(ValueError, match="mlp_precision does not support predict_normals or a normals head"):
        run(network_fine=head, predict_normals=True)
    emb_q = nerf.HashEmbedder(scene["bbox"], log2_hashmap_size=14, finest_resolution=512, use_quantization=True)
    emb_q = emb_q.to(gpu).eval()
    sh = nerf.SHEncoder()
    with pytest.raises(ValueError, match="A-CAQ quantizers are not supported"):
        run(network_query_fn=lambda p, v, fn: nerf.run_network(p, v, fn, emb_q, sh), embed_fn=emb_q)
    with pytest.raises(ValueError, match="A-CAQ quantizers are not supported"):     # caught by the field call
        run(network_query_fn=lambda p, v, fn: nerf.run_network(p, v, fn, emb_q, sh), embed_fn=None)
    # a query function that does not reach this package's run_network must not render unpacked, or in fp32, silently
    foreign = lambda p, v, fn: torch.zeros(p.shape[0], p.shape[1], 4, device=p.device)   # noqa: E731
    with pytest.raises(ValueError, match="mlp_precision needs a network_query_fn that calls this package's run_"):
        run(network_query_fn=foreign)
    grid = scene["grid_of"](ball_mask())
    with pytest.raises(ValueError, match="mlp_precision needs a network_query_fn"):
        run(march=grid, march_samples=16, retraw=False,
            network_query_fn=lambda p, v, fn: torch.zeros(p.shape[0], 4, device=p.device))
    # render() refuses even when no chunk reaches render_rays (every ray misses an empty grid)
    empty = scene["grid_of"](ball_mask() & False)
    missed = run(ray_bounds=empty)
    assert not bool(missed["ray_hit"].any())
    with pytest.raises(ValueError, match="render: feature_precision must be"):
        run(ray_bounds=empty, feature_precision="half")
    with pytest.raises(ValueError, match="render: " + needs):
        run(ray_bounds=empty, mlp_precision=None)
    # training is untouched: the keyword's default under gradients is the call without it
    with torch.enable_grad():
        out = nerf.render_rays(scene["packed"](0)[:8], **scene["ray_kw"](feature_precision=None))
    assert out["rgb_map"].shape == (8, 3) and bool(torch.isfinite(out["rgb_map"]).all())
