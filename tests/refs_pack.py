"""Plain torch restatements of the 16-bit weight and activation packs (stedm_pack_*, stedm_space_to_depth16; include/stedm_hip.h), written
from the header's layout formulas: an index gather from the fp32 filter, one rounding, nothing else. No kernel code is imported; everything
runs on CPU tensors. Shared by tests/test_pack_refs_cpu.py (pins these functions against independent statements: a reshape / permute that
undoes each layout, refs_conv.subpixel_fold, the convolution a derived filter must reproduce) and tests/test_gpu_pack_exact.py (pins the
kernels against these, word for word).

A pack reads a LOGICAL filter L[n][c][tap] (fp32): row n of the GEMM's weight matrix, contracted channel c, tap = ky * ks + kx. A plain OIHW
filter gives L = w.reshape(O, I, taps); the dgrad filter of the training step is L[n = forward cin][c = forward cout][tap reversed]. How a
strided source maps onto L is the caller's business (logical() below restates the header's sn / sc / flip rule); every layout function takes L.

Rounding is torch's own: .half() / .bfloat16(), round to nearest even, subnormals kept. The lo word of a split value is round(v - float(hi))
(the subtraction is exact in fp32). Words are compared as int16, so +0 / -0 and the lo of a subnormal count."""
import torch

DT = {"f16": torch.float16, "bf16": torch.bfloat16}


def words(v, prec):
    """fp32 -> the int16 words of its 16-bit rounding"""
    return v.to(DT[prec]).view(torch.int16)


def hi_lo(v, prec):
    """(hi words, lo words) of the split v = hi + lo"""
    hi = v.to(DT[prec])
    return hi.view(torch.int16), (v - hi.float()).to(DT[prec]).view(torch.int16)


def logical(w, sn, sc, flip, cout, cin, taps):
    """L[n][c][tap] = w.flatten()[n * sn + c * sc + (flip ? taps - 1 - tap : tap)] (stedm_pack_conv_weight_strided)"""
    n, c, t = torch.meshgrid(torch.arange(cout), torch.arange(cin), torch.arange(taps), indexing="ij")
    return w.flatten()[n * sn + c * sc + (taps - 1 - t if flip else t)]


def oihw(w):
    """the logical filter of a plain OIHW (or [O][I][1]) weight"""
    return w.reshape(w.shape[0], w.shape[1], -1)


# ------------------------------------------------------------------------------------------------ layouts (fp32 in, fp32 out: round after)
def planes(L):
    """[n][tap][c]: the hi / lo planes of stedm_pack_conv_weight"""
    return L.permute(0, 2, 1).contiguous()


def kofs(g, taps):
    """channel offset of lane group g = lane >> 4 inside a 32-channel chunk of the 16x16x32 order: 8 g for a 1x1, 16 (g & 1) + 8 (g >> 1)
    for a filter with taps (3x3, and the 2x2 derived filters)"""
    return 8 * g if taps == 1 else 16 * (g & 1) + 8 * (g >> 1)


def _gather(L, n, c, tap):
    cout = L.shape[0]
    Lp = torch.cat([L, L.new_zeros((int(n.max()) + 1 - cout,) + tuple(L.shape[1:]))]) if int(n.max()) >= cout else L
    return Lp[n, c, tap]


def frag32(L):
    """32x32x16 order (stedm_pack_conv_weight_frag): out[tn][chunk][tap][q][lane][e] =
    L[n = tn * 128 + (q >> 1) * 64 + (q & 1) * 32 + (lane & 31)][c = chunk * 16 + (lane >> 5) * 8 + e][tap], rows beyond cout zero"""
    cout, cin, taps = L.shape
    assert cin % 16 == 0
    shape = ((cout + 127) // 128, cin // 16, taps, 4, 64, 8)
    tn, ch, tap, q, lane, e = torch.meshgrid(*[torch.arange(s) for s in shape], indexing="ij")
    return _gather(L, tn * 128 + (q >> 1) * 64 + (q & 1) * 32 + (lane & 31), ch * 16 + (lane >> 5) * 8 + e, tap)


def frag16(L):
    """16x16x32 order (stedm_pack_conv_weight_frag16): out[tn][chunk32][tap][c][lane][e] =
    L[n = tn * 128 + c * 16 + (lane & 15)][ci = chunk * 32 + kofs(lane >> 4) + e][tap], rows beyond cout zero"""
    cout, cin, taps = L.shape
    assert cin % 32 == 0
    shape = ((cout + 127) // 128, cin // 32, taps, 8, 64, 8)
    tn, ch, tap, c, lane, e = torch.meshgrid(*[torch.arange(s) for s in shape], indexing="ij")
    return _gather(L, tn * 128 + c * 16 + (lane & 15), ch * 32 + kofs(lane >> 4, taps) + e, tap)


# ------------------------------------------------------------------------------------------------ derived filters
def subpixel_taps(par, tap):
    """(dy0, dy1, dx0, dx1): the 3x3 rows and columns that land on low-res neighbour tap = a * 2 + b for output parity par = py * 2 + px"""
    def rng(p, a):
        return ((0, 0), (1, 2))[a] if p == 0 else ((0, 1), (2, 2))[a]
    return rng(par >> 1, tap >> 1) + rng(par & 1, tap & 1)


def subpixel(w):
    """OIHW 3x3 -> [4 parities][O][I][4 taps] (a logical filter per parity), summed as the kernels sum: from 0.f, dy outer, dx inner, each
    step one fp32 add"""
    O, I = w.shape[:2]
    out = w.new_zeros((4, O, I, 4))
    for par in range(4):
        for tap in range(4):
            dy0, dy1, dx0, dx1 = subpixel_taps(par, tap)
            v = w.new_zeros((O, I))
            for dy in range(dy0, dy1 + 1):
                for dx in range(dx0, dx1 + 1):
                    v = v + w[:, :, dy, dx]
            out[par, :, :, tap] = v
    return out


def up_planes(w):
    """[4 * O][4][I], parity-major (stedm_pack_conv_weight_up)"""
    return subpixel(w).permute(0, 1, 3, 2).reshape(4 * w.shape[0], 4, w.shape[1]).contiguous()


def up_frag(w, order):
    """[4 parities] + the fragment order of each parity's 2x2 filter (stedm_pack_conv_weight_up_frag, _up_frag16_hl)"""
    return torch.stack([order(Lp) for Lp in subpixel(w)])


def s2d_tap(par, tap, pad_br):
    """(dy, dx) of the 3x3 filter that tap = a * 2 + b of the 2x2 filter applies to parity block par = py * 2 + px of the space-to-depth
    planes, negative = none. Pad 1 on every side: plane rows (y - 1, y) hold image rows 2y - 2 .. 2y + 1, the filter covers 2y - 1 .. 2y + 1.
    pad_br: plane rows (y, y + 1) hold image rows 2y .. 2y + 3, the filter covers 2y .. 2y + 2."""
    def one(p, a):
        if pad_br:
            return p if a == 0 else (2 if p == 0 else -1)
        return (0 if p == 1 else -1) if a == 0 else (1 if p == 0 else 2)
    return one(par >> 1, tap >> 1), one(par & 1, tap & 1)


def s2d(w, pad_br):
    """OIHW 3x3 stride 2 -> the logical 2x2 filter over the planes, [O][4 * I][4 taps], channel = parity block * I + c"""
    O, I = w.shape[:2]
    out = w.new_zeros((O, 4, I, 4))
    for par in range(4):
        for tap in range(4):
            dy, dx = s2d_tap(par, tap, pad_br)
            if dy >= 0 and dx >= 0:
                out[:, par, :, tap] = w[:, :, dy, dx]
    return out.reshape(O, 4 * I, 4)


def space_to_depth(x):
    """NHWC [B][H][W][C] -> [B][H/2][W/2][4C], channel block py * 2 + px = pixel (2y + py, 2x + px) (stedm_space_to_depth16)"""
    B, H, W, C = x.shape
    return x.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4 * C).contiguous()


def conv2x2_ref(p, L, pad_br):
    """the 2x2 stride-1 convolution the s2d filter is read by: out (y, x) = sum over taps (a, b) of plane pixel (y + a - 1, x + b - 1)
    (pad_br: (y + a, x + b)), zero outside, times L[:, :, a * 2 + b]. One matmul per tap."""
    B, H, W, C = p.shape
    o = 0 if pad_br else 1
    pp = p.new_zeros((B, H + 1, W + 1, C))
    pp[:, o:o + H, o:o + W] = p
    acc = None
    for a in range(2):
        for b in range(2):
            t = pp[:, a:a + H, b:b + W].reshape(-1, C) @ L[:, :, a * 2 + b].t()
            acc = t if acc is None else acc + t
    return acc.view(B, H, W, L.shape[0])
