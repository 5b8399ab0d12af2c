"""GPU tier (-m gpu): the attention kernels of the U-Net in the qkv-first order of the qkv plane (STEDM_ATTN_QKV_FIRST: QKVAttention,
openaimodel.py:401-428; entry points stedm_attn_qkv / stedm_attn_qkv16 / stedm_attn_qkv_bwd, ops.attn_legacy* with order=1).

A (sample, head) problem is the same arithmetic in both orders, only three base addresses differ. So, on the cases, selector patterns,
tier-2 inputs and per-element bounds of tests/refs_attn.py (the ones tests/test_gpu_attn_exact.py holds the heads-first kernels to):
  * the order-1 result on refs_attn_order.order_pack(q, k, v) is bit-equal to the order-0 result on refs_attn.legacy_pack(q, k, v);
  * it is exact on every selector pattern and inside refs_attn.tier2_bound on the random operands;
  * backward: d_qkv of order 1 is the re-laid-out d_qkv of order 0 bit for bit, and it is autograd of the restated QKVAttention
    (refs_attn_order.qkv_attention_new) under the bound tests/test_gpu_train.py holds the heads-first backward to (2e-5 of the largest entry);
  * every buffer lies between sentinel bytes that must survive, outputs start as NaN (an element nobody wrote shows), inputs stay as they were;
  * an order outside {0, 1} is an argument error (StedmHipError) of all three entries.
"""
import pytest
import torch

from tests import refs_attn as R
from tests import refs_attn_order as O

pytestmark = pytest.mark.gpu

torch.set_grad_enabled(False)

NANW = 0x7FFF              # a NaN in f16 and in bf16
I16 = torch.int16
GUARD = 256                # sentinel bytes on each side of a buffer (keeps the 256-B alignment of the allocation)
MARK = 0xA5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stedm_amd import _lib
    _lib.lib()  # must load: no fallback
    return torch.device("cuda:0")


class Guarded:
    """device copies of host tensors between sentinel bytes; check(): the sentinels are intact, the inputs unchanged"""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def put(self, x, keep=True):
        x = x.contiguous()
        nb = x.numel() * x.element_size()
        raw = torch.full((nb + 2 * GUARD,), MARK, dtype=torch.uint8, device=self.dev)
        raw[GUARD:GUARD + nb] = x.view(-1).view(torch.uint8).to(self.dev)
        view = raw[GUARD:GUARD + nb].view(x.dtype).view(x.shape)
        assert view.data_ptr() % 16 == 0
        self.bufs.append((raw, nb, x.clone() if keep else None, view))
        return view

    def out(self, shape, dtype, fill):
        return self.put(torch.full(shape, fill, dtype=dtype), keep=False)

    def check(self, tag):
        for i, (raw, nb, orig, view) in enumerate(self.bufs):
            assert bool((raw[:GUARD] == MARK).all()) and bool((raw[GUARD + nb:] == MARK).all()), f"{tag}: sentinel of buffer {i} overwritten"
            if orig is not None:
                assert torch.equal(view.cpu().view(torch.uint8), orig.view(torch.uint8)), f"{tag}: input buffer {i} changed"


def _prec(name):
    from stedm_amd import ops
    pr = ops.Precision.parse(name)
    assert (pr.mm_dtype, pr.npass) == {"f16": (ops.F16, 1), "bf16": (ops.BF16, 1)}[name]
    return pr


def _runner(dev, order, B, T, heads, ch, precision, plane):
    """precision None: the fp32 kernel; else the 16-bit forms from the int16 plane (plane) or fp32 rows"""
    from stedm_amd import ops

    def run(q, k, v):
        qkv = O.pack(order, q, k, v, B, heads)
        g = Guarded(dev)
        if precision is None:
            out = g.out((B, T, heads * ch), torch.float32, float("nan"))
            ops.attn_legacy(g.put(qkv.float()), out, heads, order=order)
            res = out.cpu().double()
        else:
            dt = R.DTYPES[precision]
            assert torch.equal(qkv.to(dt).double(), qkv)         # the operands are exact in the type: both input forms carry the same values
            src = g.put(qkv.to(dt).view(I16) if plane else qkv.float())
            out = g.out((B, T, heads * ch), I16, NANW)
            ops.attn_legacy16(src, out, heads, _prec(precision), order=order)
            res = out.cpu().view(dt).double()
        torch.cuda.synchronize()
        g.check(f"order {order}")
        bad = (~torch.isfinite(res)).any(-1).nonzero()
        assert bad.numel() == 0, f"order {order}: NaN / inf (or an output element never written) in {bad.shape[0]} rows, first {bad[0].tolist()}"
        return R.legacy_unpack(res, B, heads)
    return run


def _selectors(P, T, ch):
    """the selector cases of tests/test_gpu_attn_exact.py"""
    sel = [("one_hot",) + tuple(R.one_hot(P, T, ch, seed=T + ch)[:4]), ("group",) + tuple(R.group(P, T, ch, seed=T + ch)[:4])]
    if T > 64:
        sel.append(("late",) + tuple(R.late(P, T, ch, seed=T + ch)[:4]))
    if ch >= 32:
        sel.append(("below_zero",) + tuple(R.below_zero(P, T, ch, seed=T + ch)[:4]))
    return sel


def _check(tag, kernel, precision, dev, B, T, heads, ch, plane=True):
    new = _runner(dev, 1, B, T, heads, ch, None if precision == "fp32" else precision, plane)
    old = _runner(dev, 0, B, T, heads, ch, None if precision == "fp32" else precision, plane)
    for name, q, k, v, ex in _selectors(B * heads, T, ch):
        got = new(q, k, v)
        bad = (got != ex).any(-1).nonzero()
        assert bad.numel() == 0, f"{tag} {name}: {bad.shape[0]} wrong rows, first (problem, query) {bad[0].tolist()}"
        assert torch.equal(got, old(q, k, v)), f"{tag} {name}: order 1 differs from order 0"
    q, k, v = R.tier2_inputs(kernel, precision, B * heads, T, ch, seed=7 * T + ch)
    r = R.legacy_ref(q, k, v)
    R.assert_spread(r)
    got = new(q, k, v)
    assert torch.equal(got, old(q, k, v)), f"{tag}: order 1 on order_pack differs from order 0 on legacy_pack (random operands)"
    ratio = float(((got - r["out"]).abs() / R.tier2_bound(kernel, precision, r, q, k, v, T, ch)).max())
    print(f"[{tag} order 1] selectors exact, bit-equal to order 0; tier 2 worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio
    # the plane of the other order is another problem: the layouts are told apart
    if heads > 1:
        swapped = _runner(dev, 0, B, T, heads, ch, None if precision == "fp32" else precision, plane)
        qs, ks, vs = O.legacy_unpack_qkv(O.order_pack(q, k, v, B, heads), B, heads)
        assert not torch.equal(swapped(qs, ks, vs), got)


@pytest.mark.parametrize("B,T,heads,ch", R.CASES["attn_legacy"])
def test_attn_fp32_order1(dev, B, T, heads, ch):
    _check(f"attn_legacy fp32 B{B} T{T} h{heads} ch{ch}", "attn_legacy", "fp32", dev, B, T, heads, ch)


@pytest.mark.parametrize("plane", [False, True], ids=["fp32rows", "int16plane"])
@pytest.mark.parametrize("precision", ["f16", "bf16"])
@pytest.mark.parametrize("B,T,heads,ch", R.CASES["attn64"])
def test_attn64_mfma_order1(dev, B, T, heads, ch, precision, plane):
    assert T == 64 and ch in (32, 64, 128) and (B * heads) % 4 != 0         # attn64_mfma_kernel<T, ch, plane, 1>, a workgroup with dead waves
    _check(f"attn64_mfma {precision} ch{ch} {'int16 plane' if plane else 'fp32 rows'}", "attn64", precision, dev, B, T, heads, ch, plane)


@pytest.mark.parametrize("precision", ["f16", "bf16"])
@pytest.mark.parametrize("B,T,heads,ch", R.CASES["attn_flash"])
def test_attn_flash_order1(dev, B, T, heads, ch, precision):
    assert T != 64 and not (T >= 1024 and ch == 128)                          # attn_flash_kernel<T, ch, 4, 2, 1>
    _check(f"attn_flash {precision} B{B} T{T} h{heads} ch{ch}", "attn_flash", precision, dev, B, T, heads, ch)


def test_attn_flash_eight_wave_form_order1(dev):
    """attn_flash_kernel<T, 128, 8, 4, 1> (T >= 1024, ch = 128, enough workgroups to fill the chip): bit-equal to order 0 and inside the
    bound on random operands - one case, the size at which the entry picks that form"""
    from stedm_amd import ops
    B, T, heads, ch = 8, 1024, 8, 128
    assert B * heads * (T // 256) >= 256
    q, k, v = R.tier2_inputs("attn_flash", "f16", B * heads, T, ch, seed=11)
    outs = []
    for order in (1, 0):
        g = Guarded(dev)
        src = g.put(O.pack(order, q, k, v, B, heads).to(torch.float16).view(I16))
        out = g.out((B, T, heads * ch), I16, NANW)
        ops.attn_legacy16(src, out, heads, _prec("f16"), order=order)
        torch.cuda.synchronize()
        g.check(f"eight-wave order {order}")
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    P = 3                                                       # the bound on three problems: first, one in the middle, last
    idx = torch.tensor([0, B * heads // 2 + 1, B * heads - 1])
    r = R.legacy_ref(q[idx], k[idx], v[idx])
    got = R.legacy_unpack(outs[0].view(torch.float16).double(), B, heads)[idx]
    ratio = float(((got - r["out"]).abs() / R.tier2_bound("attn_flash", "f16", r, q[idx], k[idx], v[idx], T, ch)).max())
    print(f"[attn_flash 8-wave order 1] bit-equal to order 0; worst err / bound {ratio:.3f} on {P} problems")
    assert ratio <= 1.0


def test_unknown_order_is_an_argument_error(dev):
    from stedm_amd import ops
    from stedm_amd._lib import StedmHipError
    B, T, heads, ch = 1, 64, 2, 32
    qkv = torch.zeros(B, T, 3 * heads * ch, device=dev)
    out = torch.zeros(B, T, heads * ch, device=dev)
    for order in (2, -1):
        with pytest.raises(StedmHipError, match="order"):
            ops.attn_legacy(qkv, out, heads, order=order)
        with pytest.raises(StedmHipError, match="order"):
            ops.attn_legacy16(qkv, torch.zeros(B, T, heads * ch, dtype=I16, device=dev), heads, _prec("f16"), order=order)
        with pytest.raises(StedmHipError, match="order"):
            ops.attn_legacy_bwd(qkv, out, torch.zeros_like(qkv), heads, order=order)
    torch.cuda.synchronize()


# (2,64,2,32), (2,64,8,128): attn64_bwd_mfma_kernel; (2,64,2,16), (3,100,2,16): attn_legacy_bwd_kernel (LDS-resident);
# (1,130,2,16): attn_bwd_rows_kernel + attn_bwd_cols_kernel over the workspace, last row block of 2 queries, last column block of 2 keys
BWD_CASES = [(2, 64, 2, 32, "mfma"), (2, 64, 8, 128, "mfma"), (2, 64, 2, 16, "lds"), (3, 100, 2, 16, "lds"), (1, 130, 2, 16, "ws")]


@pytest.mark.parametrize("B,T,heads,ch,form", BWD_CASES)
def test_attention_backward_order1(dev, B, T, heads, ch, form):
    from stedm_amd import _lib, ops
    nws = _lib.lib().stedm_attn_legacy_bwd_ws_floats(B, T, heads)
    assert (nws > 0) == (form == "ws") and (form != "mfma" or (T == 64 and ch % 32 == 0)) and (form != "lds" or not (T == 64 and ch % 32 == 0))
    if form == "ws":
        assert T % 32 == 2                                     # QT = 32 query rows per block, 32 key columns per block: 2 left over in each
    g_ = torch.Generator().manual_seed(T + heads)
    q, k, v = (torch.randn(B * heads, T, ch, generator=g_) for _ in range(3))
    d = torch.randn(B, T, heads * ch, generator=g_)
    res = {}
    for order in (0, 1):
        qkv = O.pack(order, q, k, v, B, heads)
        g = Guarded(dev)
        dq = g.out(tuple(qkv.shape), torch.float32, float("nan"))
        ops.attn_legacy_bwd(g.put(qkv), g.put(d), dq, heads, order=order)
        torch.cuda.synchronize()
        g.check(f"backward order {order}")
        res[order] = dq.cpu()
        assert bool(torch.isfinite(res[order]).all()), f"order {order}: d_qkv element never written"
    assert torch.equal(res[1], O.relayout(res[0], B, heads, O.QKV_FIRST)), "d_qkv of order 1 is not the re-laid-out d_qkv of order 0"
    x = O.order_pack(q, k, v, B, heads).permute(0, 2, 1).clone().requires_grad_(True)          # the reference's layout [B][3 heads ch][T]
    with torch.enable_grad():
        y = O.qkv_attention_new(x, heads)                                                       # [B][heads ch][T]
        (y * d.permute(0, 2, 1)).sum().backward()
    ref = x.grad.permute(0, 2, 1)
    err = float((res[1] - ref).abs().max() / ref.abs().max())
    print(f"[attn backward order 1 B{B} T{T} h{heads} ch{ch} {form}] bit-equal to order 0 re-laid-out; vs autograd {err:.2e}")
    assert err < 2e-5, err
