"""GPU tier (-m gpu): style path — set-ViT encoder (patch embed, LSA flash attention with diagonal mask, MLP, pooled
head), aggregation blocks and the layout SpatialRescaler — against the reference's golden vectors and the CPU oracle."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from stedm_amd.utils import prng

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rel(a, b):
    a = a.double().cpu(); b = torch.as_tensor(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) / (float(b.std()) + 1e-12)


def make_svit(dev, img, ns, precision="parity"):
    from stedm_amd.style import sViT
    m = sViT(image_size=img, patch_size=8, num_classes=512, dim=256, depth=6, heads=12, mlp_dim=256, pool="mean", channels=3,
             dropout=0.1, emb_dropout=0.1, ns=ns, t_dim=256, precision=precision).eval()
    prng.fill_module_(m, seed=7)
    for l, (attn, _ff) in enumerate(m.transformer.layers):
        attn.fn.temperature.fill_(float(np.log(64 ** -0.5)) + 0.05 * l)
    return m.to(dev)


def test_svit_state_dict_names(dev):
    from oracle import style as ost
    from stedm_amd.style import sViT
    m = sViT(image_size=64, patch_size=8, num_classes=512, dim=256, depth=6, heads=12, mlp_dim=256, pool="mean", ns=4)
    shapes = ost.svit_shapes(ost.SViTConfig(image_size=64, ns=4))
    sd = m.state_dict()
    assert set(sd) == set(shapes)
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(shapes[k]), k


@pytest.mark.parametrize("tag,img,ns,B", [("i64_ns1", 64, 1, 2), ("i64_ns4", 64, 4, 2)])
def test_svit_vs_reference_golden(dev, golden, tag, img, ns, B):
    fx = golden("f7_svit")
    m = make_svit(dev, img, ns)
    x = prng.uniform(7, f"svit.{tag}.img", (B, ns, img, img, 3)).to(dev)
    y = m(x)
    err = rel(y, fx[tag])
    print(f"[sViT {tag}] parity-mode rel err vs reference golden: {err:.3e}")
    assert err < 1e-3


def test_svit_512_vs_reference_golden(dev, golden):
    """Full-size style encoder: 4 images of 512x512 -> 4098 tokens (the reference materialises 12 x 4098^2 logits)."""
    fx = golden("f7_svit")
    m = make_svit(dev, 512, 4)
    x = prng.uniform(7, "svit.i512_ns4.img", (1, 4, 512, 512, 3)).to(dev)
    y = m(x)
    err = rel(y, fx["i512_ns4"])
    print(f"[sViT 512 ns4] parity-mode rel err vs reference golden: {err:.3e}")
    assert err < 1e-3


@pytest.mark.parametrize("precision,tol", [("f16", 1e-2), ("bf16", 8e-2)])
def test_svit_fast_modes_reported(dev, golden, precision, tol):
    fx = golden("f7_svit")
    m = make_svit(dev, 64, 4, precision)
    x = prng.uniform(7, "svit.i64_ns4.img", (2, 4, 64, 64, 3)).to(dev)
    err = rel(m(x), fx["i64_ns4"])
    print(f"[sViT i64_ns4 {precision}] rel err vs reference golden: {err:.3e}")
    assert err < tol


@pytest.mark.parametrize("precision", ["bf16", "f16"])
@pytest.mark.parametrize("nb,T,heads,dim,bias", [(2, 1026, 12, 256, False), (3, 4098, 12, 256, False), (11, 514, 4, 128, True), (1, 2050, 12, 256, True),
                                                 (12, 4098, 12, 256, False), (13, 4098, 2, 128, True)])      # the last two: enough M-tiles for the N-persistent form
def test_to_qkv_epilogue_writes_the_attention_planes(dev, precision, nb, T, heads, dim, bias):
    """to_qkv with the qkv epilogue (stedm_conv_args.qkv_*; vit_set.py:52-57) against the same GEMM with its fp32 output: q = round(out * scale),
    k = round(out), v^T = round(out) transposed — bit for bit (same accumulation order; q in fp16 to one ulp), rows / columns t >= T untouched; tiles that
    straddle two samples (T is no multiple of 256) and a ragged last tile included."""
    from stedm_amd import ops
    from stedm_amd._lib import F16
    prec = ops.Precision.parse(precision)
    ft = torch.float16 if prec.mm_dtype == F16 else torch.bfloat16
    M, N, Tp = nb * T, 3 * heads * 64, (T + 127) // 128 * 128
    x16 = (torch.randn(M, dim, device=dev) * 0.8).to(ft).view(torch.int16)
    w = torch.randn(N, dim, 1, 1, device=dev) / math.sqrt(dim)
    bs = torch.randn(N, device=dev) * 0.2 if bias else None
    whi, wlo = ops.pack_conv_weight(w, prec); wf = ops.pack_conv_weight_frag(w, prec)
    v4 = lambda t: t.view(1, 1, M, -1)
    out = torch.empty(M, N, device=dev)
    ops.conv_igemm(None, whi, wlo, v4(out), prec=prec, ks=1, src16=(v4(x16), None), w_frag=wf, bias=bs)
    i16 = torch.int16
    fill = 0x1234
    q, k = (torch.full((nb * heads, Tp, 64), fill, dtype=i16, device=dev) for _ in range(2))
    vt = torch.full((nb * heads, 64, Tp), fill, dtype=i16, device=dev)
    scale = 0.1375
    kw = dict(prec=prec, ks=1, src16=(v4(x16), None), w_frag=wf, bias=bs, qkv_planes=(q, k, vt, T, Tp, heads, scale))
    assert ops.conv_igemm(None, whi, wlo, None, query_rs=True, **kw), "the register-streamed kernel should take this problem"
    ops.conv_igemm(None, whi, wlo, None, **kw)
    o = out.view(nb, T, 3, heads, 64)
    planes = lambda s_, sc: (o[:, :, s_] * sc).to(ft).permute(0, 2, 1, 3).reshape(nb * heads, T, 64)      # [nb * heads][T][64]
    # (fp16: the scale and the conversion may be one fused multiply-convert, i.e. a single rounding of out * scale: at most one ulp from the two-step value)
    assert torch.allclose(q[:, :T].view(ft).float(), planes(0, scale).float(), rtol=1.1e-3, atol=1e-7) if ft == torch.float16 else \
        torch.equal(q[:, :T].view(ft), planes(0, scale))
    assert torch.equal(k[:, :T].view(ft), planes(1, 1.0))
    assert torch.equal(vt[:, :, :T].view(ft), planes(2, 1.0).transpose(1, 2))
    assert bool((q[:, T:] == fill).all()) and bool((k[:, T:] == fill).all()) and bool((vt[:, :, T:] == fill).all())


@pytest.mark.parametrize("precision", ["bf16", "f16"])
@pytest.mark.parametrize("M,K,N,form", [(50000, 256, 256, "out"), (50000, 256, 384, "res"), (49153, 128, 256, "o16"), (50000, 256, 256, "gelu"),
                                        (65536, 192, 128 * 5, "res"), (50000, 128, 288, "o16"), (50000, 192, 576, "gelu"), (49999, 256, 200, "res")])      # ragged last N-tile
def test_short_k_gemm_n_persistent_form_is_the_tiled_one_bit_for_bit(dev, precision, M, K, N, form):
    """The set-ViT's FeedForward / to_out style GEMMs (vit_set.py:23-31): with K <= 256 and enough M-tiles one block per M-tile walks all
    N-tiles and stores from the accumulators (conv_rs.inc, RS_1X1N) — same sums, same epilogue order as the tile-per-block form
    (STEDM_CONV_NO_NPERS=1), ragged last M-tile included; and both against a float64 product."""
    import os
    from stedm_amd import ops
    from stedm_amd._lib import F16
    prec = ops.Precision.parse(precision)
    ft = torch.float16 if prec.mm_dtype == F16 else torch.bfloat16
    x = (torch.randn(M, K, device=dev) * 0.7).to(ft)
    w = (torch.randn(N, K, 1, 1, device=dev) / math.sqrt(K)).to(ft).float()
    bs = torch.randn(N, device=dev) * 0.3
    res0 = torch.randn(M, N, device=dev)
    whi, wlo = ops.pack_conv_weight(w, prec); wf = ops.pack_conv_weight_frag(w, prec)
    v4 = lambda t: t.view(1, 1, M, -1)

    def run():
        out = res0.clone() if form == "res" else (torch.full((M, N), float("nan"), device=dev) if form == "out" else None)
        o16 = torch.full((M, N), 0x7FFF, dtype=torch.int16, device=dev) if form in ("o16", "gelu") else None
        ops.conv_igemm(None, whi, wlo, None if out is None else v4(out), prec=prec, ks=1, src16=(v4(x.view(torch.int16)), None), w_frag=wf, bias=bs,
                       res=v4(out) if form == "res" else None, act_out=2 if form == "gelu" else 0, out16=None if o16 is None else (v4(o16), None))
        return out if out is not None else o16.view(ft).float()

    got = run()
    os.environ["STEDM_CONV_NO_NPERS"] = "1"
    try:
        ref_tiled = run()
    finally:
        del os.environ["STEDM_CONV_NO_NPERS"]
    if form == "gelu" and ft == torch.float16:     # the last multiply of the GELU and the fp16 conversion may fuse into one rounding: one ulp
        assert torch.allclose(got, ref_tiled, rtol=1.1e-3, atol=1e-7)
    else:
        assert torch.equal(got, ref_tiled)
    ref = x.double() @ w.view(N, K).double().t() + bs.double()
    if form == "res": ref = ref + res0.double()
    if form == "gelu": ref = F.gelu(ref)
    assert rel(got, ref.cpu().numpy()) < (1e-5 if form in ("out", "res") else (5e-2 if precision == "bf16" else 6e-3))     # 16-bit forms: half an ulp of the largest output over the spread


@pytest.mark.parametrize("precision,tol", [("f16", 1e-2), ("bf16", 8e-2)])
def test_svit_512_fused_qkv_vs_reference_golden(dev, golden, precision, tol):
    """The full-size encoder (T = 4098) in the single-product modes: the to_qkv GEMMs run with the qkv epilogue (the small fixtures fall back to
    the pack pass: too few tiles for the register-streamed kernel); against the reference golden and against the unfused path."""
    fx = golden("f7_svit")
    m = make_svit(dev, 512, 4, precision)
    x = prng.uniform(7, "svit.i512_ns4.img", (1, 4, 512, 512, 3)).to(dev)
    assert m.fuse_qkv
    y = m(x).clone()
    assert not any(k_[0] in ("qkv16", "qkv") for k_ in m._bufs), "the fused path allocates no [M][3 * heads * 64] tensor"
    m.fuse_qkv = False
    y0 = m(x).clone()
    err, err0 = rel(y, fx["i512_ns4"]), rel(y0, fx["i512_ns4"])
    print(f"[sViT 512 ns4 {precision}] rel err vs reference golden: fused qkv epilogue {err:.3e}, pack pass {err0:.3e}")
    assert err < tol and err0 < tol


@pytest.mark.parametrize("B,T,heads", [(2, 66, 12), (1, 130, 2), (1, 300, 3)])
def test_lsa_flash_vs_oracle(dev, B, T, heads):
    """LSA core (vit_set.py:56-66) alone: logits * exp(tau), diagonal masked, softmax, @ v."""
    from stedm_amd import ops
    prec = ops.Precision.parse("parity")
    qkv = prng.normal(40, "lsa.qkv", (B, T, 3 * heads * 64))
    tau = math.exp(math.log(64 ** -0.5) + 0.1)
    q, k, v = (t.reshape(B, T, heads, 64).permute(0, 2, 1, 3) for t in qkv.chunk(3, dim=-1))
    dots = torch.matmul(q, k.transpose(-1, -2)) * tau
    dots = dots.masked_fill(torch.eye(T, dtype=torch.bool), -torch.finfo(dots.dtype).max)
    ref = torch.matmul(dots.softmax(dim=-1), v).permute(0, 2, 1, 3).reshape(B, T, heads * 64)
    Tp = ((T + 127) // 128) * 128
    i16 = torch.int16
    mk = lambda shp: (torch.zeros(shp, dtype=i16, device=dev), torch.zeros(shp, dtype=i16, device=dev))
    qd, kd, vd = mk((B * heads, Tp, 64)), mk((B * heads, Tp, 64)), mk((B * heads, 64, Tp))
    ops.qkv_pack(qkv.to(dev).contiguous(), tau * math.log2(math.e), qd, kd, vd, B, T, Tp, heads, prec)   # lsa_flash works in log2
    od = mk((B, T, heads * 64))
    ops.lsa_flash(qd, kd, vd, od, B, T, Tp, heads, prec)
    got = od[0].view(torch.float16).float() + od[1].view(torch.float16).float()
    assert rel(got, ref) < 2e-4


@pytest.mark.parametrize("precision,tol", [("f16", 6e-3), ("bf16", 4e-2)])
def test_lsa_flash_rising_logits_take_the_redo_path(dev, precision, tol):
    """The 64-queries-per-wave kernel has no per-tile row maximum: it exponentiates relative to a reference fixed on the first tile and redoes
    a block's tile (reference moved to the tile's maximum) when a row sum shows that the operand type cannot carry the probabilities — fp16:
    sums above 2^14; bf16: 2^80. Keys whose logits GROW along the sequence (here by ~40 in log2 units from the first tile to the last,
    past fp16's range, with a jump beyond 2^80 for bf16 at the end) must come out as with a running maximum."""
    from stedm_amd import ops
    prec = ops.Precision.parse(precision)
    B, T, heads = 1, 600, 2
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, T, heads, 64, generator=g)
    kk = torch.randn(B, T, heads, 64, generator=g)
    v = torch.randn(B, T, heads, 64, generator=g)
    # every key gets a component along the queries' mean direction that grows with its index: logits rise steadily along the sequence
    qdir = torch.nn.functional.normalize(q.mean(1, keepdim=True), dim=-1)
    q = q + 6.0 * qdir
    ramp = torch.linspace(0.0, 5.0, T).view(1, T, 1, 1)
    if precision == "bf16":
        ramp = ramp + (torch.arange(T).view(1, T, 1, 1) >= 560).float() * 14.0        # a late jump past 2^80
    kk = kk + ramp * qdir
    qkv = torch.cat([q.reshape(B, T, -1), kk.reshape(B, T, -1), v.reshape(B, T, -1)], dim=-1).contiguous()
    tau = 1.0
    # reference on the ROUNDED operands (what qkv_pack hands the kernel: q * tau * log2(e), k, v in the operand type): logits this large
    # magnify the operands' own rounding, which is not what is tested here
    dt = torch.float16 if precision == "f16" else torch.bfloat16
    rq = (q * (tau * math.log2(math.e))).to(dt).double().permute(0, 2, 1, 3)
    rk, rv = kk.to(dt).double().permute(0, 2, 1, 3), v.to(dt).double().permute(0, 2, 1, 3)
    dots = torch.matmul(rq, rk.transpose(-1, -2))
    dots = dots.masked_fill(torch.eye(T, dtype=torch.bool), -1e300)
    pr = torch.exp2(dots - dots.max(-1, keepdim=True)[0])
    ref = (torch.matmul(pr, rv) / pr.sum(-1, keepdim=True)).permute(0, 2, 1, 3).reshape(B, T, heads * 64).float()
    spread = float(dots[..., 500:].max() - dots[..., :64].max())
    assert spread > (90 if precision == "bf16" else 25), spread                       # the case really leaves the first tile's range
    Tp = ((T + 127) // 128) * 128
    mk = lambda shp: (torch.zeros(shp, dtype=torch.int16, device=dev), None)
    qd, kd, vd = mk((B * heads, Tp, 64)), mk((B * heads, Tp, 64)), mk((B * heads, 64, Tp))
    ops.qkv_pack(qkv.to(dev), tau * math.log2(math.e), qd, kd, vd, B, T, Tp, heads, prec)
    od = mk((B, T, heads * 64))
    ops.lsa_flash(qd, kd, vd, od, B, T, Tp, heads, prec)
    got = od[0].view(dt).float()
    assert bool(torch.isfinite(got).all())
    err = rel(got, ref)
    print(f"[lsa_flash rising logits {precision}] spread {spread:.0f} (log2 units), max|diff|/std {err:.3e}")
    assert err < tol


def test_agg_blocks_vs_reference_golden(dev, golden):
    import types
    from stedm_amd import style as st
    fx = golden("f8_agg")

    class StandIn(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.proj = torch.nn.Linear(3 * 4 * 4, 512)

        def forward(self, x):
            return self.proj(F.adaptive_avg_pool2d(x, 4).flatten(1))

    samp = types.SimpleNamespace(name="mp", num_patches=4)
    sty = prng.uniform(8, "agg.style", (2, 4, 16, 16, 3)).to(dev)
    for name, cls in (("mean", st.Agg_Mean), ("max", st.Agg_Max), ("linear", st.Agg_Linear)):
        m = cls(samp, StandIn()).eval()
        sd = {k: prng.fill_value(8, k, v.shape) for k, v in m.state_dict().items() if not k.startswith("_")}
        m.load_state_dict(sd, strict=False)
        y = m.to(dev)(sty)
        assert rel(y, fx[name]) < 2e-5, name
    assert torch.equal(st.Agg_None(samp, None)(sty).cpu(), torch.from_numpy(fx["none"]))


def test_spatial_rescaler_vs_reference_golden(dev, golden):
    from stedm_amd.style import SpatialRescaler
    fx = golden("f9_rescaler")
    m = SpatialRescaler(n_stages=2, in_channels=2, out_channels=3).eval()
    prng.fill_module_(m, seed=9)
    seg = (prng.uniform(9, "resc.seg", (2, 2, 64, 64)) > 0).float()
    y = m.to(dev)(seg.to(dev))
    assert rel(y, fx["y"]) < 2e-6
    assert rel(m.encode(seg.to(dev)), fx["y"]) < 2e-6


@pytest.mark.parametrize("tag,img,B", [("i64_ns8", 64, 2), ("i512_ns8", 512, 1)])
def test_svit_eight_style_images_vs_reference_golden(dev, golden, tag, img, B):
    """BASELINE config 5: 8 style inputs through the set encoder (patch features 192 * 8 = 1536 wide): the reference's own sViT(ns=8)
    (tests/golden/make_golden_ns8.py), incl. the full 512^2 / 4098-token case. parity mode < 1e-3."""
    fx = golden("f7_svit_ns8")
    m = make_svit(dev, img, 8)
    x = prng.uniform(7, f"svit.{tag}.img", (B, 8, img, img, 3)).to(dev)
    err = rel(m(x), fx[tag])
    print(f"[sViT {tag}] parity-mode rel err vs reference golden: {err:.3e}")
    assert err < 1e-3


@pytest.mark.parametrize("src16", [False, True])
@pytest.mark.parametrize("B,H,T", [(2, 3, 300), (1, 2, 66), (1, 1, 700)])
def test_lsa_flash_mx8_kernel(dev, B, H, T, src16):
    """the MX-fp8 attention (e4m3 bytes, one E8M0 scale per 32 elements, v_mfma_scale_f32_32x32x64_f8f6f4). Two checks:
    (i) the pack pass is bit-exact against a torch restatement of the format (scales from the block maxima, bytes by round-to-nearest e4m3,
        V^T with the tile's keys in the kernel's contraction order);
    (ii) the attention on the DEQUANTISED operands in fp64 agrees with the kernel to what P's e4m3 rounding leaves (checks the operand lane
        maps, the per-lane scales, the masks, the reference / redo rule), and the deviation from the fp32 attention on the original q, k, v —
        what the format costs — is reported."""
    from stedm_amd import ops
    pr = ops.Precision.parse("fp8")
    Tp = ((T + 127) // 128) * 128
    qkv = prng.normal(41, f"mx8.qkv.{T}", (B, T, 3 * H * 64))
    qkv[:, T // 2:, H * 64:2 * H * 64] *= 3.0          # keys whose logits outgrow the first tile's reference: the redo rule runs
    tau = 0.125 * 1.4426950408889634
    if src16:
        src = qkv.to(torch.bfloat16)
        qkv = src.float()
        dsrc = src.view(torch.int16).to(dev)
    else:
        dsrc = qkv.to(dev)
    u8 = torch.uint8
    q8 = torch.zeros((B * H, Tp, 64), dtype=u8, device=dev); k8 = torch.zeros_like(q8); v8 = torch.zeros((B * H, 64, Tp), dtype=u8, device=dev)
    qs = torch.zeros((B * H, Tp, 2), dtype=u8, device=dev); ks = torch.zeros_like(qs); vs = torch.zeros((B * H, Tp // 32, 64), dtype=u8, device=dev)
    out16 = torch.zeros((B, T, H * 64), dtype=torch.int16, device=dev)
    ops.qkv_pack_mx8(dsrc, tau, q8, qs, k8, ks, v8, vs, B, T, Tp, H, pr)
    ops.lsa_flash_mx8(q8, qs, k8, ks, v8, vs, out16, B, T, Tp, H, pr)
    got = out16.view(torch.bfloat16).float().cpu()
    assert bool(torch.isfinite(got).all())
    # ---- (i) the format, restated
    q, k, v = (t.reshape(B, T, H, 64).permute(0, 2, 1, 3).reshape(B * H, T, 64) for t in qkv.split(H * 64, dim=-1))
    pad = lambda t: torch.cat([t, t.new_zeros(t.shape[0], Tp - T, 64)], 1)
    q, k, v = pad(q * tau), pad(k), pad(v)

    from tests.refs_attn import mx, mx_deq as deq, mx_keys      # the format, restated: (e4m3 tensor, scale exponents) per 32 elements
    qb_, qe = mx(q.reshape(B * H, Tp, 2, 32)); kb_, ke = mx(k.reshape(B * H, Tp, 2, 32))
    assert torch.equal(q8.cpu().view(torch.float8_e4m3fn).view(u8), qb_.reshape(B * H, Tp, 64).view(u8)) and torch.equal(qs.cpu().int() - 127, qe.int())
    assert torch.equal(k8.cpu().view(u8), kb_.reshape(B * H, Tp, 64).view(u8)) and torch.equal(ks.cpu().int() - 127, ke.int())
    keys = mx_keys()                                                                                     # [block h][j] -> key inside the tile (position 32 h + j)
    vt = v.reshape(B * H, Tp // 64, 64, 64)[:, :, keys, :]                                               # [bh][kt][h][j][d]
    vb_, ve = mx(vt.permute(0, 1, 2, 4, 3).contiguous())                                                  # blocks [bh][kt][h][d][32]
    want_v8 = vb_.permute(0, 3, 1, 2, 4).reshape(B * H, 64, Tp)                                           # [bh][d][kt*64 + h*32 + j]
    assert torch.equal(v8.cpu().view(u8), want_v8.contiguous().view(u8)) and torch.equal(vs.cpu().int().reshape(B * H, Tp // 64, 2, 64) - 127, ve.int())
    # ---- (ii) attention on the dequantised operands, fp64
    qd = deq(qb_, qe).reshape(B * H, Tp, 64)[:, :T]; kd = deq(kb_, ke).reshape(B * H, Tp, 64)[:, :T]
    vd_perm = deq(vb_, ve)                                                                                # [bh][kt][h][d][j]
    vd = torch.zeros(B * H, Tp // 64, 64, 64, dtype=torch.float64)                                        # [bh][kt][key][d]
    vd[:, :, keys, :] = vd_perm.permute(0, 1, 2, 4, 3)
    vd = vd.reshape(B * H, Tp, 64)[:, :T]
    logits = qd @ kd.transpose(-1, -2)                                                                    # log2 domain (tau carries log2 e)
    logits.diagonal(dim1=-2, dim2=-1).fill_(-1e300)
    pr_ = torch.exp2(logits - logits.amax(-1, keepdim=True))
    ref_q = ((pr_ @ vd) / pr_.sum(-1, keepdim=True)).reshape(B, H, T, 64).permute(0, 2, 1, 3).reshape(B, T, H * 64)
    lq = float((got.double() - ref_q).norm() / ref_q.norm())
    q0, k0, v0 = (t.reshape(B, T, H, 64).permute(0, 2, 1, 3).double() for t in qkv.split(H * 64, dim=-1))
    l0 = (q0 @ k0.transpose(-1, -2)) * 0.125
    l0.diagonal(dim1=-2, dim2=-1).fill_(-1e300)
    ref = (l0.softmax(-1) @ v0).permute(0, 2, 1, 3).reshape(B, T, H * 64)
    l2 = float((got.double() - ref).norm() / ref.norm())
    print(f"[lsa_flash_mx8 B{B} H{H} T{T} src16={src16}] rel-L2 vs attention on the dequantised operands {lq:.3e} (P's e4m3 rounding), vs fp32 attention {l2:.3e}")
    assert lq < 4e-2 and l2 < 1e-1


def test_svit_fp8_attention_mode_reported(dev, golden):
    """BASELINE config 5's numerics mode: sViT with e4m3 attention operands (everything else bf16 single product) vs the reference golden —
    deviation reported next to the bf16 mode's, not asserted at 1e-3."""
    fx = golden("f7_svit_ns8")
    x = prng.uniform(7, "svit.i64_ns8.img", (2, 8, 64, 64, 3)).to(dev)
    res = {}
    for precision in ("bf16", "fp8"):
        m = make_svit(dev, 64, 8, precision)
        y = m(x)
        a, b = y.double().cpu(), torch.from_numpy(fx["i64_ns8"]).double()
        res[precision] = float((a - b).norm() / b.norm())
        assert bool(torch.isfinite(y).all())
    print(f"[sViT ns=8, 64^2] rel-L2 vs reference golden: bf16 {res['bf16']:.3e}, bf16 + fp8 attention {res['fp8']:.3e}")
    assert res["fp8"] < 0.2 and res["bf16"] < 0.05


def test_svit_fp8_attention_at_config5_size_vs_reference_golden(dev, golden):
    """BASELINE config 5's style half at its own size: 8 style images of 512 x 512 -> T = 4098 tokens, 12 heads x 64,
    the LSA attention (vit_set.py:52-67) on v_mfma_scale_f32_32x32x64_f8f6f4 with MX-fp8 operands, everything else bf16 single product -
    against the reference's own output (F7 `i512_ns8`, tests/golden/make_golden_ns8.py). Measured (round 5): bf16 3.2e-3, MX-fp8 4.0e-3 rel-L2
    (averaging over 4098 keys hides most of e4m3's 3 mantissa bits). Bounds: bf16 < 1e-2, fp8 < 1.5e-2 and within 2x of bf16's + 5e-3; finite.
    A reported mode - the tolerance mode of the encoder is `parity` (test_svit_ns8_vs_reference_golden)."""
    fx = golden("f7_svit_ns8")
    x = prng.uniform(7, "svit.i512_ns8.img", (1, 8, 512, 512, 3)).to(dev)
    ref = torch.from_numpy(fx["i512_ns8"]).double()
    res = {}
    for precision in ("bf16", "fp8"):
        m = make_svit(dev, 512, 8, precision)
        y = m(x)
        assert bool(torch.isfinite(y).all())
        res[precision] = float((y.double().cpu() - ref).norm() / ref.norm())
    print(f"[sViT ns=8, 512^2, T=4098] rel-L2 vs reference golden: bf16 {res['bf16']:.3e}, bf16 + MX-fp8 attention {res['fp8']:.3e}")
    assert res["bf16"] < 1e-2 and res["fp8"] < 1.5e-2 and res["fp8"] < 2 * res["bf16"] + 5e-3


# ------------------------------------------------------------------------------------------------ train-mode dropout (vit_set.py:28-30, 43/62, 49, 187)
def test_dropout_rows_matches_the_mask_stream(dev):
    """Elementwise sites: the kernel's keep mask is the specified Philox stream bit for bit; kept values carry torch's 1 / (1 - p) scale; the
    residual add and the 16-bit operand planes follow; a ragged tail (n % 8 != 0) is handled."""
    from oracle import dropmask as dm
    from stedm_amd import ops
    prec = ops.Precision.parse("parity")
    for n, p, seed, site in [(8 * 4099 + 5, 0.1, 0x1234567890ABCDEF, 19), (1 << 16, 0.25, 7, 0x10000), (24, 0.1, 3, 1)]:
        src = prng.normal(61, f"drop.src.{n}", (n,))
        res = prng.normal(61, f"drop.res.{n}", (n,))
        keep = torch.from_numpy(dm.keep_elementwise(n, p, seed, site))
        scale = torch.tensor(1.0) / torch.tensor(1.0 - np.float32(p))
        want = torch.where(keep, src * scale, torch.zeros_like(src))
        out = torch.empty(n, device=dev)
        ops.dropout_rows(src.to(dev), p, seed, site, prec, out=out)
        assert torch.equal(out.cpu(), want), "mask or scale differs from the stream's definition"
        hi, lo = torch.empty(n, dtype=torch.int16, device=dev), torch.empty(n, dtype=torch.int16, device=dev)
        x = res.to(dev).clone()
        ops.dropout_rows(src.to(dev), p, seed, site, prec, res=x, out=x, hi=hi, lo=lo)          # in place on the residual stream
        assert torch.equal(x.cpu(), want + res)
        planes = hi.view(torch.float16).float() + lo.view(torch.float16).float()
        assert float((planes.cpu() - (want + res)).abs().max()) < 1e-5
    # keep-rate statistics of a large draw: thr16 = round(0.1 * 65536) = 6554
    n = 1 << 22
    out = torch.empty(n, device=dev)
    ops.dropout_rows(torch.ones(n, device=dev), 0.1, 99, 5, prec, out=out)
    rate = float((out != 0).float().mean())
    assert abs(rate - (1 - 6554 / 65536)) < 4 * math.sqrt(0.09 / n), rate


def _lsa_ref(qkv, tau, heads, keep=None, p=0.0):
    B, T, _ = qkv.shape
    q, k, v = (t.reshape(B, T, heads, 64).permute(0, 2, 1, 3) for t in qkv.chunk(3, dim=-1))
    dots = torch.matmul(q, k.transpose(-1, -2)) * tau
    dots = dots.masked_fill(torch.eye(T, dtype=torch.bool), -torch.finfo(dots.dtype).max)
    attn = dots.softmax(dim=-1)
    if keep is not None:
        attn = torch.where(keep, attn / (1.0 - p), torch.zeros_like(attn))
    return torch.matmul(attn, v).permute(0, 2, 1, 3).reshape(B, T, heads * 64)


@pytest.mark.parametrize("precision,tol", [("parity", 2e-4), ("f16", 1e-2), ("bf16", 6e-2)])
@pytest.mark.parametrize("B,T,heads", [(2, 66, 12), (1, 130, 2), (1, 300, 3)])
def test_lsa_flash_drop_vs_oracle_with_the_same_mask(dev, B, T, heads, precision, tol):
    """Attention-probability dropout (vit_set.py:61-62) inside the flash kernels (the register-staged split-product one and the DMA one): the
    softmax normalises over ALL keys, the PV product sees only the kept probabilities, scaled by 1 / (1 - p). Mask = the specified per-lane
    xorshift128 streams, rebuilt in numpy; a wrong mask would show as an O(0.3) error."""
    from oracle import dropmask as dm
    from stedm_amd import ops
    prec = ops.Precision.parse(precision)
    p, seed, site = 0.1, 0xC0FFEE1234, 8 * 3 + 1
    qkv = prng.normal(40, "lsa.qkv", (B, T, 3 * heads * 64))
    tau = math.exp(math.log(64 ** -0.5) + 0.1)
    keep = torch.from_numpy(dm.keep_attention(B * heads, T, p, seed, site)).reshape(B, heads, T, T)
    ref = _lsa_ref(qkv, tau, heads, keep, p)
    Tp = ((T + 127) // 128) * 128
    i16 = torch.int16
    lo_ok = prec.npass == 3
    mk = lambda shp: (torch.zeros(shp, dtype=i16, device=dev), torch.zeros(shp, dtype=i16, device=dev) if lo_ok else None)
    qd, kd, vd = mk((B * heads, Tp, 64)), mk((B * heads, Tp, 64)), mk((B * heads, 64, Tp))
    ops.qkv_pack(qkv.to(dev).contiguous(), tau * math.log2(math.e), qd, kd, vd, B, T, Tp, heads, prec)
    od = mk((B, T, heads * 64))
    ops.lsa_flash_drop(qd, kd, vd, od, B, T, Tp, heads, prec, p, seed, site)
    dt = torch.float16 if precision != "bf16" else torch.bfloat16
    got = od[0].view(dt).float() + (od[1].view(dt).float() if lo_ok else 0)
    err = rel(got, ref)
    print(f"[lsa_flash_drop {precision} B{B} T{T} h{heads}] max|diff|/std vs oracle with the same mask: {err:.3e} "
          f"(no-dropout reference would differ by {rel(_lsa_ref(qkv, tau, heads), ref):.2f})")
    assert err < tol
    # p = 0: thr16 = 0 keeps everything and the scale is 1 -> the eval kernel's output bit for bit
    o0, o1 = mk((B, T, heads * 64)), mk((B, T, heads * 64))
    ops.lsa_flash(qd, kd, vd, o0, B, T, Tp, heads, prec)
    ops.lsa_flash_drop(qd, kd, vd, o1, B, T, Tp, heads, prec, 0.0, seed, site)
    assert torch.equal(o0[0], o1[0]) and (not lo_ok or torch.equal(o0[1], o1[1]))


def make_svit_cfg(dev, img, ns, depth, heads, precision="parity"):
    from stedm_amd.style import sViT
    m = sViT(image_size=img, patch_size=8, num_classes=512, dim=256, depth=depth, heads=heads, mlp_dim=256, pool="mean", channels=3,
             dropout=0.1, emb_dropout=0.1, ns=ns, t_dim=256, precision=precision)
    prng.fill_module_(m, seed=7)
    for l, (attn, _ff) in enumerate(m.transformer.layers):
        attn.fn.temperature.fill_(float(np.log(64 ** -0.5)) + 0.05 * l)
    return m.to(dev)


@pytest.mark.parametrize("tag,img,ns,B,depth,heads", [("i64_ns4_d2", 64, 4, 2, 2, 12), ("i32_ns1_d3", 32, 1, 3, 3, 4)])
def test_svit_train_mode_vs_reference_golden(dev, golden, tag, img, ns, B, depth, heads):
    """sViT.train() with the shipped dropout values (conf/style_agg/svit.yaml: 0.1 / 0.1) against the REFERENCE's own module in train mode
    with the same masks injected at its nn.Dropout calls (fixture F16, tests/golden/make_golden_train_drop.py)."""
    fx = golden("f16_svit_train_drop")
    m = make_svit_cfg(dev, img, ns, depth, heads).train()
    m.dropout_seed = int(fx["seed"][0])
    x = prng.uniform(7, f"svit.train.{tag}.img", (B, ns, img, img, 3)).to(dev)
    y = m(x).clone()
    err = rel(y, fx[tag])
    print(f"[sViT train {tag}] parity-mode rel err vs the reference in train mode with the same masks: {err:.3e} "
          f"(eval output differs by {rel(y, fx[tag + '.eval']):.2f})")
    assert err < 1e-3
    assert torch.equal(m(x), y), "same seed, same masks"
    assert rel(m.eval()(x), fx[tag + ".eval"]) < 1e-3
    # a forward without an explicit seed draws one from torch's generator: torch.manual_seed governs it, successive forwards differ
    m.train()
    m.dropout_seed = None
    torch.manual_seed(5)
    a = m(x).clone(); s1 = m.last_dropout_seed
    b = m(x).clone(); s2 = m.last_dropout_seed
    torch.manual_seed(5)
    c = m(x).clone()
    assert s1 != s2 and not torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("precision,tol", [("f16", 1e-2), ("bf16", 8e-2)])
def test_svit_train_mode_fast_modes_reported(dev, golden, precision, tol):
    fx = golden("f16_svit_train_drop")
    m = make_svit_cfg(dev, 64, 4, 2, 12, precision).train()
    m.dropout_seed = int(fx["seed"][0])
    x = prng.uniform(7, "svit.train.i64_ns4_d2.img", (2, 4, 64, 64, 3)).to(dev)
    err = rel(m(x), fx["i64_ns4_d2"])
    print(f"[sViT train i64_ns4_d2 {precision}] rel err vs the reference in train mode with the same masks: {err:.3e}")
    assert err < tol


def test_svit_train_mode_with_zero_dropout_is_eval_bitwise(dev):
    from stedm_amd.style import sViT
    m = sViT(image_size=64, patch_size=8, num_classes=512, dim=256, depth=2, heads=12, mlp_dim=256, pool="mean", ns=4, dropout=0.0,
             emb_dropout=0.0)
    prng.fill_module_(m, seed=7)
    m = m.to(dev)
    x = prng.uniform(7, "svit.train.p0.img", (2, 4, 64, 64, 3)).to(dev)
    assert torch.equal(m.train()(x).clone(), m.eval()(x))
