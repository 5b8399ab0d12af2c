"""Plain torch restatements of what the implicit-GEMM convolution kernels compute (stedm_conv_igemm, include/stedm_hip.h), written from the
header's formulas: a sum over taps of a shifted slice of the zero-padded input times one [cout][cin] matrix. No kernel code is imported.
Every function runs in the dtype and on the device of its inputs: fp64 for a reference, fp32 to pin a property of fp32 itself. Shared by
tests/test_conv_refs_cpu.py (pins these functions against F.conv2d) and tests/test_gpu_conv_exact.py (pins the kernels against these).

Layouts: activations NHWC [B][H][W][C]; weights [cout][taps][cin], tap = ky * ks + kx (the hi / lo planes of stedm_pack_conv_weight);
sub-pixel weights [4 parities py * 2 + px][cout][4 taps a * 2 + b][cin] (stedm_pack_conv_weight_up); outputs NHWC.

Two ways to an exact reference:
  dyadic operands (refs_bwd.dyadic): every product is a multiple of 1/64 of magnitude <= wmax, so every fp32 partial sum of k_total of them
    is exact in every order while k_total * 64 * wmax < 2^24 (dyadic_ok): any kernel form must equal the fp64 result bit for bit;
  operands read back from the 16-bit planes (as_f64): an fp64 convolution of exactly the values the kernel multiplies; the kernel's fp32
    accumulation is all that lies between the two, measured in units of u * S with S = abs_sum(...) and bounded by G (below)."""
import torch

from tests.refs_bwd import U, dyadic, normal          # noqa: F401  (re-exported: the two input generators and the fp32 unit roundoff)

# Growth factor of a plain fp32 accumulation: max |fp32 conv of the 16-bit-rounded operands - fp64| / (u * S), elementwise, at K = 2304 and
# K = 18432, f16 and bf16. G_PLAIN = 0.5 is the NOMINAL figure, not the largest measurement: torch's CPU convolution gives 0.46 .. 0.68 at
# K = 2304 and 0.37 .. 0.39 at K = 18432 (tests/test_conv_refs_cpu.py::test_growth_factor_of_a_plain_fp32_accumulation measures and prints
# them, and holds this constant to within a factor of two of the largest). The maximum over a few thousand outputs scatters with the
# sample; taking 0.5 rather than 0.68 makes the GPU tier's bound the stricter of the two (G = 8, not 10.9). The GPU tier allows 16 x
# G_PLAIN: the margin for the MFMA's internal summation order, the split-K partials and the epilogue's three additions. Neither number
# comes from a kernel.
G_PLAIN = 0.5
G = 16 * G_PLAIN

MAX_F64_BYTES = 1 << 30


def as_f64(plane_int16, prec_label):
    """the 16-bit words of an operand plane, viewed as the mode's float type ('f16...' / 'bf16...') and widened to fp64"""
    assert plane_int16.dtype == torch.int16
    return plane_int16.view(torch.float16 if prec_label.startswith("f16") else torch.bfloat16).double()


def dyadic_ok(k_total, wmax=1.0):
    """proof obligation of a bit-exact case: k_total products, each a multiple of 1/64 of magnitude <= wmax, summed in fp32"""
    assert k_total * 64 * wmax < 2 ** 24, (k_total, wmax)


def otc(w_oihw):
    """OIHW -> [O][taps][I], tap = ky * ks + kx: the layout of the weight planes and of conv_ref's second argument"""
    return w_oihw.permute(0, 2, 3, 1).reshape(w_oihw.shape[0], -1, w_oihw.shape[1]).contiguous()


def out_hw(H, W, mode):
    return (H // 2, W // 2) if mode == "down" else ((2 * H, 2 * W) if mode == "up" else (H, W))


def conv_ref(a_nhwc, w_otc, mode, ks, pad_br=False):
    """mode 's1': stride 1, pad ks // 2 (ks 3 or 1). 'down': 3x3 stride 2, pad 1 on every side, or bottom / right only (pad_br: the VQ
    encoder's Downsample, F.pad(x, (0, 1, 0, 1)) + conv(stride 2, padding 0)); H, W even. 'up': nearest 2x, then 3x3 stride 1 pad 1.
    One matmul per tap; chunked over the batch so that the padded input of a chunk stays under 1 GiB."""
    assert mode in ("s1", "down", "up") and ks in (1, 3) and (mode == "s1" or ks == 3) and (not pad_br or mode == "down")
    B, H, W, C = a_nhwc.shape
    O, taps, Cw = w_otc.shape
    assert taps == ks * ks and Cw == C
    Ho, Wo = out_hw(H, W, mode)
    st = 2 if mode == "down" else 1
    p0 = 0 if pad_br else ks // 2                       # pad before; after: whatever the last tap needs
    Hs, Ws = (2 * H, 2 * W) if mode == "up" else (H, W)
    Hp, Wp = st * (Ho - 1) + ks, st * (Wo - 1) + ks
    out = a_nhwc.new_empty((B, Ho, Wo, O))
    per = max(1, MAX_F64_BYTES // (Hp * Wp * C * a_nhwc.element_size()))
    for b0 in range(0, B, per):
        x = a_nhwc[b0:b0 + per]
        if mode == "up":
            x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
        xp = x.new_zeros((x.shape[0], max(Hp, p0 + Hs), max(Wp, p0 + Ws), C))
        xp[:, p0:p0 + Hs, p0:p0 + Ws] = x
        acc = None
        for ky in range(ks):
            for kx in range(ks):
                patch = xp[:, ky:ky + st * (Ho - 1) + 1:st, kx:kx + st * (Wo - 1) + 1:st]
                t = patch.reshape(-1, C) @ w_otc[:, ky * ks + kx, :].t()
                acc = t if acc is None else acc + t
        out[b0:b0 + per] = acc.view(-1, Ho, Wo, O)
    return out


_ROWS = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}          # parity -> 3x3 rows (columns) summed into tap 0 and tap 1


def subpixel_fold(w_oihw):
    """OIHW 3x3 -> [4 parities][O][4 taps][I]: W_eff[py][px][a][b] = the sum of the 3x3 taps that read the same low-res pixel
    (rows: py=0 -> {0},{1,2}; py=1 -> {0,1},{2}; columns by the same rule)"""
    O, I, kh, kw = w_oihw.shape
    assert kh == 3 and kw == 3
    out = w_oihw.new_zeros((4, O, 4, I))
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    for dy in _ROWS[py][a]:
                        for dx in _ROWS[px][b]:
                            out[py * 2 + px, :, a * 2 + b, :] += w_oihw[:, :, dy, dx]
    return out


def conv_ref_subpixel(a_nhwc, w_eff):
    """the four parity 2x2 convolutions on the low-res grid, interleaved: output (2y + py, 2x + px) = sum over taps (a, b) of
    input (y + a - 1 + py, x + b - 1 + px) (zero outside) times w_eff[py * 2 + px][:, a * 2 + b, :]"""
    B, H, W, C = a_nhwc.shape
    O = w_eff.shape[1]
    assert tuple(w_eff.shape) == (4, O, 4, C)
    xp = a_nhwc.new_zeros((B, H + 2, W + 2, C))
    xp[:, 1:H + 1, 1:W + 1] = a_nhwc
    out = a_nhwc.new_empty((B, 2 * H, 2 * W, O))
    for py in range(2):
        for px in range(2):
            acc = None
            for a in range(2):
                for b in range(2):
                    patch = xp[:, a + py:a + py + H, b + px:b + px + W]
                    t = patch.reshape(-1, C) @ w_eff[py * 2 + px, :, a * 2 + b, :].t()
                    acc = t if acc is None else acc + t
            out[:, py::2, px::2] = acc.view(B, H, W, O)
    return out


def epilogue(ref, bias=None, emb=None, emb_offset=0, res=None):
    """+ bias[n] + emb[b][emb_offset + n] + res, as the kernels' epilogues add them"""
    O = ref.shape[-1]
    if bias is not None:
        ref = ref + bias
    if emb is not None:
        ref = ref + emb[:, None, None, emb_offset:emb_offset + O]
    if res is not None:
        ref = ref + res
    return ref


def slot_runs(HW, run, device=None):
    """pixel -> slot for row-major runs of `run` pixels (the 256-pixel slots of the epilogues, the caller-chosen runs of a reduce pass)"""
    return torch.arange(HW, device=device) // run


def slot_parity(H, W, device=None):
    """pixel of the 2H x 2W output -> slot of the sub-pixel upsample's epilogue: (256-pixel run of the low-res pixel) * 4 + py * 2 + px"""
    y = torch.arange(2 * H, device=device)[:, None]
    x = torch.arange(2 * W, device=device)[None, :]
    return ((((y // 2) * W + (x // 2)) // 256) * 4 + (y % 2) * 2 + (x % 2)).reshape(-1)


def slab_stats(out, slab):
    """out [B][Ho][Wo][O] -> (sum, sum of squares), each [B][slots][O], in fp64. slab: pixels per slot (row-major runs) or a pixel -> slot
    index tensor (slot_runs / slot_parity)."""
    B, O = out.shape[0], out.shape[-1]
    v = out.double().reshape(B, -1, O)
    idx = slot_runs(v.shape[1], slab, v.device) if isinstance(slab, int) else slab.to(v.device)
    ns = int(idx.max()) + 1
    s = v.new_zeros((B, ns, O)).index_add_(1, idx, v)
    q = v.new_zeros((B, ns, O)).index_add_(1, idx, v * v)
    return s, q


def three_products(ah, al, wh, wl, conv):
    """what the split-product modes compute: hi.hi + hi.lo + lo.hi (lo.lo is dropped by design); conv(a, w) is the convolution at hand"""
    return conv(ah, wh) + conv(ah, wl) + conv(al, wh)


def abs_sum(a, w, conv, bias=None, emb=None, emb_offset=0, res=None):
    """the same convolution and epilogue on the magnitudes: the scale S in which a kernel's accumulated rounding error is measured"""
    ab = lambda t: None if t is None else t.abs()
    return epilogue(conv(a.abs(), w.abs()), ab(bias), ab(emb), emb_offset, ab(res))
