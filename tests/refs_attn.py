"""Plain fp64 restatements of the attention kernels (attn.hip, svit.hip, attn_fp8.hip), the per-element bound of their rounding points, the
selector inputs whose correct output is known exactly, and an fp32 emulation of each kernel's arithmetic with switchable defects. Nothing
of stedm_amd is imported. Shared by tests/test_attn_refs_cpu.py (pins the references against oracle/, proves that both tiers reject the
defects) and tests/test_gpu_attn_exact.py (pins the kernels).

Everything works on "problems": q, k, v [P][T][ch] with P = samples x heads, fp64 values that are exactly representable in the operand
type of the kernel under test (the caller rounds; for the split-product modes the value is hi + lo). `legacy_pack` / `lsa_planes` lay them
out as the entries expect.

Tier 1 (selectors). Keys and queries are sign codes c (+-1)^ch with c = 16: a dot product is 256 (ch - 2 d), d the Hamming distance, a
multiple of 512 (+ 256 ch) below 2^16: exact in fp32 in any order, and exactly representable in f16 and bf16, so even the kernels that
exponentiate relative to a reference ROUNDED to the operand type (attn_flash_kernel, lsa_flash64_kernel: move_ref) hold the row maximum
exactly. The matching key's probability is exp(0) = 1, every other key is at least GAP_NATS = 160 nats below (asserted): exp underflows
to exactly 0 in fp32. l is the number of matching keys (1, 2 or 4), 1 / l a power of two, the output a sum of at most four integers
divided by it: every kernel must return the expected value bit for bit (torch.equal), whatever its tiling, reference rule or rescale.
  one_hot: query t carries the code of key pi(t), pi a random derangement; v[s][c] = ((s + 37 c) mod 511) - 255 differs between any two
           keys in EVERY channel (T <= 511) and is exact in bf16. Expected out[t] = v[pi(t)]; a wrong key is off by >= 1 everywhere.
  group:   groups of 2 and 4 keys share a code (members in different 64-key tiles where T allows, one group holds the LAST key); v integer
           in [-4, 4]; expected the group mean (a multiple of 1/4). With the diagonal mask (LSA) the members of the groups of 2 point at
           their own group and expect the OTHER member's v.
  late:    (T > 64) every target lies behind the first 64-key tile and the whole first tile lies far below it (`late`): what a kernel does
           with a first-tile softmax reference whose exponential overflows.
  below_zero: (ch >= 32) every logit is negative (`below_zero`): a key row beyond T that holds zeros has logit 0 and would take every
           row if the tail mask let it through - the zero pad rows of LSA, of the MX planes and of the fp32 kernel are out of sight of
           the three patterns above, whose targets lie far above 0.
Swin's cosine logits are bounded by the scale (<= 100), so no selector exists there; its tier 1 is `swin_uniform` (q = 0, rpb = 0, v = the
bits of the source token's position): the output is the fraction of set bits among the visible keys, within 2 u_T.

Tier 2 (per-element bound, `bound`). Rounding points, per kernel (u = 2^-24, u_T = half an ulp of the operand type, fl = f16's
subnormal floor 2^-25; the hardware exp / rcp are taken as 2 u as in tests/refs_style.py):
  every kernel   logits: fp32 accumulation of exact products (16-bit operands) or of rounded ones (fp32 kernel, two pre-scales): absolute
                 error e_l <= (ch + 4) u max_s sum_c |q||k| (the + 4: the pre-scales or the reference k-step, the subtraction of the
                 reference, the post-scale); exponential: one multiplication by log2 e or the scale (u |x|, |x| <= the asserted spread)
                 and the hardware exp2 (2 u): e_p = expm1(e_l) + u x_max + 2 u relative on every unnormalised p. It enters the
                 numerator (e_p A) and l (e_p |ref| <= e_p A): 2 e_p A.
                 sums: O over T keys, l over T keys, one rescale (2 roundings + the exponential of alpha) per tile, 1 / l and the final
                 product: (T + 4 ntiles + 4) u (A + |ref|).
  attn_legacy_kernel (fp32)          nothing else.
  attn64_mfma_kernel, attn_flash_kernel, lsa_flash64_kernel (one product, T = f16 / bf16)
                 P rounded to T for the second product while l sums the unrounded p: u_T A + fl sum_s |v| / l_min (l_min = 1 with a row
                 maximum; 2^-(u_T max|s|) for the rounded reference, which may sit that far above the maximum); the output rounded to T:
                 u_T |out| + fl.
  lsa_flash_kernel<T, 3> (hi + lo)   logits lose lo.lo: e_l += max_s sum_c |q_lo||k_lo|; P = hi + lo pair (2 u_T^2 relative), the second
                 product loses p_lo v_lo: (u_T w) . |v_lo|; the output pair: 2 u_T^2 |out| + fl.
  lsa_flash64_mx8_kernel             as the one-product form with u_T = 2^-4 for e4m3 P (bf16 output: + 2^-8 |out|); the floor is e4m3's
                 subnormal half-spacing 2^-10 of the bytes 16 p, i.e. 2^-14 per key; the reference is not rounded (l_min = 1).
A[t][c] = sum_s w[t][s] |v[s][c]| with the (dropout-scaled) softmax weights w. No factor is fitted; what is not derived here is not in the
bound. Tier-2 inputs keep every row's logit spread under 20 log2 units (`assert_spread` on the reference of every case).
"""
import math

import torch

from tests.refs_style import U, plane_terms

F64 = torch.float64
F32 = torch.float32
GAP_NATS = 160.0
CODE = 16.0
FLT_MAX = 3.4028234663852886e38
LOG2E = 1.4426950408889634
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "parity": torch.float16, "parity_bf16": torch.bfloat16, "fp8": torch.float8_e4m3fn}


def u_of(dtype):
    """(half an ulp of the 16-bit type, its absolute floor); (0, 0) for fp32 outputs; e4m3: 2^-4"""
    if dtype is None:
        return 0.0, 0.0
    if dtype == torch.float8_e4m3fn:
        return 2.0 ** -4, 2.0 ** -14       # the bytes carry 16 p: e4m3's subnormal spacing 2^-9, half of it, over 16
    _, h, fl = plane_terms(dtype)
    return h, fl


# ------------------------------------------------------------------------------------------------ references
def attention_ref(q, k, v, scale, base2=False, diag=False, keep=None, p=0.0):
    """softmax(scale q k^T [log2 domain: 2^x]) v in fp64 on the operands as given. diag: a token does not attend to itself. keep [P][T][T]
    bool: kept probabilities scaled by 1 / (1 - p), the normalisation l keeps every p.
    Returns dict(out, A = w |v|, lmag = max_s scale sum_c |q||k| per row, smax = max_s |logit| per row, spread, w)."""
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    if diag:
        s = s.masked_fill(torch.eye(s.shape[-1], dtype=torch.bool), -math.inf)
    m = s.amax(-1, keepdim=True)
    e = torch.exp2(s - m) if base2 else torch.exp(s - m)
    w = e / e.sum(-1, keepdim=True)
    if keep is not None:
        w = torch.where(keep, w / (1.0 - p), torch.zeros_like(w))
    fin = torch.where(torch.isfinite(s), s, m.expand_as(s))
    unit = 1.0 if base2 else LOG2E
    return dict(out=torch.matmul(w, v), A=torch.matmul(w, v.abs()), w=w,
                lmag=(torch.matmul(q.abs(), k.abs().transpose(-1, -2)) * scale).amax(-1, keepdim=True),
                unit=unit, smax=fin.abs().amax(-1, keepdim=True), spread=float((m - fin.amin(-1, keepdim=True)).max()) * unit,
                vsum=v.abs().sum(-2, keepdim=True))


def legacy_ref(q, k, v):
    """QKVAttentionLegacy on problems [P][T][ch]: the scale 1 / sqrt(ch) on the product"""
    return attention_ref(q, k, v, 1.0 / math.sqrt(q.shape[-1]))


def lsa_ref(q, k, v, keep=None, p=0.0):
    """LSA core: q carries tau log2(e) (as qkv_pack delivers it), diagonal masked, log2 domain"""
    return attention_ref(q, k, v, 1.0, base2=True, diag=True, keep=keep, p=p)


def bound(r, T, ch, dtype, *, npass=1, ref_rounded=False, lo=None, out_dtype="same", tile=64):
    """the per-element bound of the module docstring for a result dict r of attention_ref. dtype: type of P (None: fp32 kernel).
    ref_rounded: the kernel exponentiates relative to a reference rounded to dtype. lo = (q_lo, k_lo, v_lo) magnitudes for npass 3."""
    uT, fl = u_of(dtype)
    out, A = r["out"].abs(), r["A"]
    nt = (T + tile - 1) // tile
    unit = 1.0 / LOG2E                                   # r['spread'] is in log2 units; the exponent's argument in nats
    e_l = (ch + 4) * U * r["lmag"]
    if npass == 3:
        ql, kl, vl = lo
        e_l = e_l + torch.matmul(ql.abs(), kl.abs().transpose(-1, -2)).amax(-1, keepdim=True)
    e_p = torch.expm1(e_l * (r["unit"] / LOG2E)) + U * (r["spread"] * unit + 1.0) + 2 * U
    b = 2 * e_p * A + (T + 4 * nt + 4) * U * (A + out)
    if dtype is None:
        return b
    od = dtype if out_dtype == "same" else out_dtype
    uo, flo = u_of(od)
    if npass == 3:
        b = b + 2 * uT * uT * A + torch.matmul(uT * r["w"], vl.abs()) + fl * r["vsum"]
        return b + 2 * uo * uo * (out + b) + flo
    lmin = torch.exp2(-uT * r["smax"] * r["unit"]) if ref_rounded else 1.0
    b = b + uT * A + fl * r["vsum"] / lmin
    return b + uo * (out + b) + flo


# ------------------------------------------------------------------------------------------------ layouts
def legacy_pack(q, k, v, B, heads):
    """problems [B*heads][T][ch] -> qkv [B][T][heads * 3 * ch], channel = head * 3 ch + {q: 0, k: ch, v: 2 ch} + c"""
    P, T, ch = q.shape
    x = torch.stack([q, k, v], 2).reshape(B, heads, T, 3 * ch)
    return x.permute(0, 2, 1, 3).reshape(B, T, heads * 3 * ch).contiguous()


def legacy_unpack(out, B, heads):
    """out [B][T][heads * ch] -> [B*heads][T][ch]"""
    _, T, C = out.shape
    return out.reshape(B, T, heads, C // heads).permute(0, 2, 1, 3).reshape(B * heads, T, C // heads)


def lsa_planes(q, k, v, Tp, dtype, lo=False):
    """problems [P][T][64] -> ((q_hi, q_lo), (k_hi, k_lo), (vt_hi, vt_lo)) int16 planes [P][Tp][64] / [P][64][Tp], rows / columns >= T zero;
    lo planes (the 16-bit rounding of the fp32 remainder) only when asked"""
    P, T, ch = q.shape

    def planes(x, tr):
        xp = torch.zeros((P, Tp, ch), dtype=F64)
        xp[:, :T] = x
        if tr:
            xp = xp.transpose(1, 2).contiguous()
        hi = xp.to(dtype)
        l_ = (xp - hi.double()).to(dtype)
        return (hi.view(torch.int16), l_.view(torch.int16) if lo else None)
    return planes(q, False), planes(k, False), planes(v, True)


def split_lo(x, dtype):
    """(hi, lo) of an fp64 tensor as fp64: hi the rounding to dtype, lo the rounding of the remainder"""
    hi = x.to(dtype).double()
    return hi, (x - hi).to(dtype).double()


# ------------------------------------------------------------------------------------------------ MX-fp8 format (attn_fp8.hip, include/stedm_hip.h)
def mx(x):
    """x [..., 32] -> (e4m3 tensor, scale exponents): one E8M0 scale per 32 elements from the block maximum, bytes by round-to-nearest"""
    amax = x.abs().amax(-1)
    e = torch.where(amax > 0, torch.frexp(amax / 448.0)[1], torch.full_like(amax, -127, dtype=torch.int32)).clamp(-127, 127)
    y = (x * torch.ldexp(torch.ones_like(amax), -e).unsqueeze(-1)).to(torch.float8_e4m3fn)
    return y, e


def mx_keys():
    """[block h][j] -> key inside the 64-key tile at position 32 h + j of the V^T contraction order"""
    j = torch.arange(32)
    return torch.stack([32 * h + ((j & 15) >> 2) * 8 + 4 * (j >> 4) + (j & 3) for h in range(2)])


def mx_deq(y, e):
    """the fp64 values an MX block stands for"""
    return y.double() * torch.ldexp(torch.ones_like(e, dtype=F64), e).unsqueeze(-1)


# ------------------------------------------------------------------------------------------------ inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def random_qkv(P, T, ch, dtype, seed, logit_std=2.0, base2=False, npass=1):
    """tier-2 operands: N(0, 1) v, q and k scaled so that the logits have standard deviation ~logit_std (log2 units for base2), rounded to
    dtype (npass 3: to the hi + lo pair). Returns fp64 problems (q, k, v); the caller's reference asserts the spread."""
    g = _gen(seed)
    q = torch.randn(P, T, ch, generator=g, dtype=F64)
    k = torch.randn(P, T, ch, generator=g, dtype=F64)
    v = torch.randn(P, T, ch, generator=g, dtype=F64)
    if base2:
        q = q * (logit_std / math.sqrt(ch))
    else:
        f = math.sqrt(logit_std / LOG2E)                  # logits = q k / sqrt(ch) in nats: standard deviation f^2
        q, k = q * f, k * f

    def rnd(x):
        if dtype is None:
            return x.float().double()
        if npass == 3:
            h, l_ = split_lo(x.float().double(), dtype)
            return h + l_
        return x.to(dtype).double()
    return rnd(q), rnd(k), rnd(v)


def assert_spread(r):
    assert r["spread"] < 20.0, r["spread"]


def codes(T, ch, seed, tries=8, groups=()):
    """[T][ch] sign codes c (+-1)^ch, distinct except inside `groups` (lists of key indices that share a code); the best of a few seeds by
    minimum Hamming distance between different codes. Returns (codes fp64, min distance)."""
    best = None
    for i in range(tries):
        g = _gen(seed * 131 + i)
        c = (torch.randint(0, 2, (T, ch), generator=g) * 2 - 1).double()
        gid = torch.arange(T)
        for grp in groups:
            c[grp] = c[grp[0]].clone()
            gid[grp] = grp[0]
        d = (ch - c @ c.t()) / 2
        d = d.masked_fill(gid[:, None] == gid[None, :], float(ch))
        dmin = int(d.min())
        if best is None or dmin > best[1]:
            best = (c * CODE, dmin)
    return best


def check_selector(q, k, scale_nats, diag=False):
    """the generator's obligations: every raw dot product exact in fp32 (integers below 2^24); in every row the best key(s) lead every other
    visible key by >= GAP_NATS. Returns the smallest gap in nats."""
    s = torch.matmul(q, k.transpose(-1, -2))
    assert bool((s == s.round()).all()) and float(s.abs().max()) * q.shape[-1] < 2 ** 24
    assert bool((s.float().double() == s).all()) and bool((s.to(torch.bfloat16).double() == s).all()), "logits must be exact in the operand types"
    if diag:
        s = s.masked_fill(torch.eye(s.shape[-1], dtype=torch.bool), -math.inf)
    m = s.amax(-1, keepdim=True)
    rest = s.masked_fill(s == m, -math.inf).amax(-1, keepdim=True)
    gap = float(((m - rest) * scale_nats).min())
    assert gap >= GAP_NATS, gap
    return gap


def _derangement(T, g):
    while True:
        p = torch.randperm(T, generator=g)
        if bool((p != torch.arange(T)).all()):
            return p


def one_hot(P, T, ch, seed):
    """(q, k, v, expected, target): query t holds the code of key pi(t)"""
    qs, ks, vs, ex, tg = [], [], [], [], []
    s_ = torch.arange(T)[:, None]
    c_ = torch.arange(ch)[None, :]
    v = (((s_ + 37 * c_) % 511) - 255).double()
    assert T <= 511
    for p in range(P):
        c, dmin = codes(T, ch, seed + 977 * p)
        assert dmin >= 1
        pi = _derangement(T, _gen(seed + 31 * p + 5))
        vp = v.roll(p, 1)
        qs.append(c[pi]); ks.append(c); vs.append(vp); ex.append(vp[pi]); tg.append(pi)
    return torch.stack(qs), torch.stack(ks), torch.stack(vs), torch.stack(ex), torch.stack(tg)


def group_layout(T):
    """groups of 4 and 2 key indices, members in different 64-key tiles where T allows; the first group of 2 holds the last key"""
    nt = (T + 63) // 64
    groups = [[3, T - 1]]
    used = {3, T - 1}
    for gi, n in enumerate((4, 2, 4, 2, 2)):
        grp = []
        for i in range(n):
            for tile in list(range((i * nt) // n, -1, -1)) + list(range((i * nt) // n + 1, nt)):      # the wanted tile, else the nearest with room
                free = [s for s in range(tile * 64, min(T, tile * 64 + 64)) if s not in used]
                if free:
                    s = free[(5 + 11 * gi + 7 * i) % len(free)]
                    grp.append(s)
                    used.add(s)
                    break
        assert len(grp) == n
        groups.append(sorted(grp))
    return groups


def group(P, T, ch, seed, diag=False):
    """(q, k, v, expected, groups): every query points at a group; with diag the members of a group of 2 point at their own group"""
    groups = group_layout(T)
    qs, ks, vs, ex = [], [], [], []
    for p in range(P):
        g = _gen(seed + 13 * p)
        c, dmin = codes(T, ch, seed + 977 * p + 1, groups=groups)
        assert dmin >= 1
        v = torch.randint(-4, 5, (T, ch), generator=g).double()
        pick = torch.randint(0, len(groups), (T,), generator=g)
        member = torch.full((T,), -1, dtype=torch.long)
        for gi, grp in enumerate(groups):
            member[grp] = gi
        q = torch.empty(T, ch, dtype=F64)
        e = torch.empty(T, ch, dtype=F64)
        for t in range(T):
            gi = int(pick[t])
            if member[t] >= 0:
                own = groups[int(member[t])]
                if diag and len(own) == 2:
                    gi = int(member[t])
                else:                                     # never its own group: the mean over three of four would not be exact
                    while gi == int(member[t]):
                        gi = (gi + 1) % len(groups)
            grp = [s for s in groups[gi] if not (diag and s == t)]
            q[t] = c[groups[gi][0]]
            e[t] = v[grp].mean(0)
        assert bool((e * 4 == (e * 4).round()).all())
        qs.append(q); ks.append(c); vs.append(v); ex.append(e)
    return torch.stack(qs), torch.stack(ks), torch.stack(vs), torch.stack(ex), groups


def late(P, T, ch, seed, diag=False):
    """(q, k, v, expected, first): every query's target lies behind the first 64-key tile, and the whole first tile lies far BELOW it: half
    of the channels are -c in the keys of the first tile and +c in every query and every later key, so a first-tile logit is at most
    `first` <= -1024 while the target's is 256 ch. A kernel that sets its softmax reference on the first tile must carry a first-tile maximum
    whose exponential (relative to 0) overflows - the rows come out as NaN if it rescales its still-empty sums by it. T > 64."""
    assert T > 64 and ch >= 32
    half, nl = ch // 2, T - 64
    s_ = torch.arange(T)[:, None]
    c_ = torch.arange(ch)[None, :]
    v = (((s_ + 37 * c_) % 511) - 255).double()
    t = torch.arange(T)
    tg = 64 + (7 * t + 3) % nl
    if diag:
        tg = torch.where(tg == t, 64 + (tg - 64 + 1) % nl, tg)
        assert nl >= 2
    qs, ks, ex, first = [], [], [], -math.inf
    for p in range(P):
        g = _gen(seed + 77 * p)
        free = (torch.randint(0, 2, (T, half), generator=g) * 2 - 1).double()
        idx = torch.arange(nl)
        bits = torch.stack([(idx >> b) & 1 for b in range(9)], 1)
        free[64:, :9] = (bits * 2 - 1).double()                         # later keys: pairwise distinct, the parity channel makes the distance >= 2
        free[64:, 9] = ((bits.sum(1) % 2) * 2 - 1).double()
        free[:64, 9] = -(((free[:64, :9] > 0).sum(1) % 2) * 2 - 1).double()      # first tile: the wrong parity and the other sign in channel 10,
        free[64:, 10], free[:64, 10] = 1.0, -1.0                                 # so no first-tile key comes nearer than distance 2 to a later code
        k = torch.cat([torch.where(s_ < 64, -1.0, 1.0).expand(T, half), free], 1) * CODE
        q = k[tg].clone()
        q[:, :half] = CODE
        first = max(first, float((q @ k[:64].t()).max()))
        qs.append(q); ks.append(k); ex.append(v[tg])
    assert first <= -1024.0, first
    return torch.stack(qs), torch.stack(ks), v.expand(P, T, ch).contiguous(), torch.stack(ex), first


def below_zero(P, T, ch, seed, diag=False):
    """(q, k, v, expected, target): EVERY logit is negative - ch / 2 + 2 channels are +c in every key and -c in every query, the other
    channels hold the target's code, so the target's logit is -1024 and every other key's at most -1024 - 512 d. A key row beyond T that
    holds zeros (logit 0, v 0: the LSA planes, the fp32 kernel's tile) would outrank every real key if the tail mask let it through: the
    output would be 0, not v[target]. ch >= 32."""
    assert ch >= 32 and T <= 511
    f = ch // 2 + 2
    free_n = ch - f
    s_ = torch.arange(T)[:, None]
    c_ = torch.arange(ch)[None, :]
    v = (((s_ + 37 * c_) % 511) - 255).double()
    idx = torch.arange(T)
    bits = torch.stack([(idx >> b) & 1 for b in range(9)], 1)
    qs, ks, ex, tgs = [], [], [], []
    for p in range(P):
        g = _gen(seed + 59 * p)
        free = (torch.randint(0, 2, (T, free_n), generator=g) * 2 - 1).double()
        free[:, :9] = (bits * 2 - 1).double()                           # pairwise distinct, the parity channel makes the distance >= 2
        free[:, 9] = ((bits.sum(1) % 2) * 2 - 1).double()
        k = torch.cat([torch.ones(T, f, dtype=F64), free], 1) * CODE
        tg = _derangement(T, g)
        q = k[tg].clone()
        q[:, :f] = -CODE
        assert float((q @ k.t()).max()) == -1024.0
        qs.append(q); ks.append(k); ex.append(v[tg]); tgs.append(tg)
    return torch.stack(qs), torch.stack(ks), v.expand(P, T, ch).contiguous(), torch.stack(ex), torch.stack(tgs)


def selector_expected(q, k, v, diag=False, keep=None, inv_keep=1.0):
    """what a selector input must give, exactly: the (kept, scaled) mean of v over the keys that tie for the row maximum"""
    s = torch.matmul(q, k.transpose(-1, -2))
    if diag:
        s = s.masked_fill(torch.eye(s.shape[-1], dtype=torch.bool), -math.inf)
    sel = s == s.amax(-1, keepdim=True)
    n = sel.sum(-1, keepdim=True).double()
    assert bool(((n == 1) | (n == 2) | (n == 4)).all())
    if keep is not None:
        sel = sel & keep
    return torch.matmul(sel.double() * inv_keep, v) / n


def mx_problem_operands(q8, qs, k8, ks, v8, vs, T):
    """the fp64 problems [P][T][64] that the MX-fp8 planes of qkv_pack_mx8 stand for (bytes uint8 [P][Tp][64] / [P][64][Tp], scale bytes
    [P][Tp][2] / [P][Tp / 32][64])"""
    P, Tp, _ = q8.shape
    e4 = torch.float8_e4m3fn
    qd = mx_deq(q8.view(e4).reshape(P, Tp, 2, 32), qs.int() - 127).reshape(P, Tp, 64)[:, :T]
    kd = mx_deq(k8.view(e4).reshape(P, Tp, 2, 32), ks.int() - 127).reshape(P, Tp, 64)[:, :T]
    vb = v8.view(e4).reshape(P, 64, Tp // 64, 2, 32).permute(0, 2, 3, 1, 4)                  # [bh][kt][h][d][j]
    vd_perm = mx_deq(vb, vs.int().reshape(P, Tp // 64, 2, 64) - 127)
    vd = torch.zeros(P, Tp // 64, 64, 64, dtype=F64)                                         # [bh][kt][key][d]
    vd[:, :, mx_keys(), :] = vd_perm.permute(0, 1, 2, 4, 3)
    return qd, kd, vd.reshape(P, Tp, 64)[:, :T]


def mx_quantise(q, k, v):
    """what qkv_pack_mx8 (scale 1) makes of problems [P][T][64], as the fp64 values its planes stand for: q, k in blocks of 32 channels, v in
    blocks of the 32 keys of a sub-tile per channel (V^T in the contraction order of mx_keys), rows beyond T zero"""
    P, T, ch = q.shape
    Tp = (T + 127) // 128 * 128
    pad = lambda t: torch.cat([t.float(), t.new_zeros(P, Tp - T, ch).float()], 1)
    qd, kd = (mx_deq(*mx(pad(x).reshape(P, Tp, 2, 32))).reshape(P, Tp, ch)[:, :T] for x in (q, k))
    vt = pad(v).reshape(P, Tp // 64, 64, ch)[:, :, mx_keys(), :]                                 # [bh][kt][h][j][d]
    vd_perm = mx_deq(*mx(vt.permute(0, 1, 2, 4, 3).contiguous()))                                 # [bh][kt][h][d][j]
    vd = torch.zeros(P, Tp // 64, 64, ch, dtype=F64)
    vd[:, :, mx_keys(), :] = vd_perm.permute(0, 1, 2, 4, 3)
    return qd, kd, vd.reshape(P, Tp, ch)[:, :T]


def lsa_qkv_rows(q, k, v, B, heads):
    """problems [B*heads][T][64] -> qkv rows [B][T][3 * heads * 64] (thirds q | k | v, head-major inside a third: what to_qkv writes)"""
    T = q.shape[1]
    f = lambda x: x.reshape(B, heads, T, 64).permute(0, 2, 1, 3).reshape(B, T, heads * 64)
    return torch.cat([f(q), f(k), f(v)], -1).contiguous()


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels' arithmetic
KLIMIT = {torch.float16: 16384.0, torch.bfloat16: 1.2089258e24, torch.float8_e4m3fn: 448.0}
E4M3 = torch.float8_e4m3fn
MUTANTS = ("drop_last", "double_key", "swap_v", "mask_off_by_one", "skip_rescale", "no_diag", "first_rescale")


def emulate(q, k, v, *, form, dtype, npass=1, pre=1.0, post=1.0, base2=False, diag=False, keep=None, inv_keep=1.0, pad="zero", tile=64,
            mutant=None, mkey=None):
    """fp32 restatement of a kernel on problems [P][T][ch] (fp64 in, fp64 out of the values the kernel stores).
    form 'online': running row maximum per `tile` keys (attn_legacy_kernel, lsa_flash_kernel; tile >= T: attn64_mfma_kernel), p =
    exp((s - m) post); 'mref': reference = the first tile's maximum rounded to dtype, moved (rounded again) when a row sum exceeds what
    the type carries (attn_flash_kernel, lsa_flash64_kernel), per row. pre: factor on q and k before the product (fp32 kernel).
    dtype: type of the operands and of P (None: fp32); npass 3: hi + lo operands, three products, hi + lo output.
    pad: what a key row beyond T holds - 'zero' (LSA planes) or 'last' (attn_flash_kernel re-reads row T - 1).
    dtype e4m3 (lsa_flash64_mx8_kernel, form 'mref'): q, k, v are the values the MX planes stand for (mx_quantise); the exponentials are
    16 p = exp2(s - reference + 4) (the + 4 rides in the accumulator), their bytes are the e4m3 rounding of 16 p, l sums the unrounded 16 p,
    the reference is NOT rounded, a tile is redone when its sum of 16 p exceeds 448, the output is bf16.
    mutant: one of MUTANTS; mkey: the key (or pair of keys) it acts on."""
    P, T, ch = q.shape
    rt = (lambda x: x) if dtype is None else (lambda x: x.to(dtype).to(F32))
    mx8 = dtype == E4M3
    rt_ref = (lambda x: x) if mx8 else rt
    rt_out = (lambda x: x.to(torch.bfloat16).to(F32)) if mx8 else rt
    shift = torch.tensor(4.0 if mx8 else 0.0, dtype=F32)
    log2e = torch.tensor(LOG2E, dtype=F32)
    ex = (lambda x: torch.exp2(x)) if base2 else (lambda x: torch.exp2(x * log2e))       # __expf(x) = v_exp_f32(x log2 e)
    nt = (T + tile - 1) // tile
    Tp = nt * tile
    q32, k32, v32 = (q.float() * torch.tensor(pre, dtype=F32)), (k.float() * torch.tensor(pre, dtype=F32)), v.float()
    if Tp > T:
        fill = (lambda x: x[:, T - 1:T].expand(P, Tp - T, ch)) if pad == "last" else (lambda x: x.new_zeros(P, Tp - T, ch))
        k32, v32 = torch.cat([k32, fill(k32)], 1), torch.cat([v32, fill(v32)], 1)
    if npass == 3:
        qh, kh, vh = rt(q32), rt(k32), rt(v32)
        ql, kl, vl = rt(q32 - qh), rt(k32 - kh), rt(v32 - vh)
    valid = T
    if mutant == "drop_last":
        valid = T - 1
    if mutant == "mask_off_by_one":
        valid = T + 1
    post_t = torch.tensor(post, dtype=F32)
    m = torch.full((P, T, 1), -math.inf, dtype=F32) if form == "online" else torch.zeros((P, T, 1), dtype=F32)
    l = torch.zeros((P, T, 1), dtype=F32)
    o = torch.zeros((P, T, ch), dtype=F32)
    skipped = False
    rows = torch.arange(T)[:, None]
    for kt in range(nt):
        sl = slice(kt * tile, (kt + 1) * tile)
        kidx = torch.arange(kt * tile, (kt + 1) * tile)[None, :]
        if npass == 3:
            s = qh @ kl[:, sl].transpose(1, 2) + ql @ kh[:, sl].transpose(1, 2) + qh @ kh[:, sl].transpose(1, 2)
        else:
            s = q32 @ k32[:, sl].transpose(1, 2)
        vt = (vh[:, sl], vl[:, sl]) if npass == 3 else (v32[:, sl], None)
        if mutant == "swap_v" and mkey[0] // tile == kt:
            a, b = mkey[0] % tile, mkey[1] % tile
            vt = tuple(None if x is None else x.clone() for x in vt)
            for x in vt:
                if x is not None:
                    x[:, [a, b]] = x[:, [b, a]]
        if diag and mutant != "no_diag":
            s = torch.where(kidx == rows, torch.tensor(-FLT_MAX, dtype=F32), s)
        s = torch.where(kidx >= valid, torch.tensor(-math.inf, dtype=F32), s)
        if form == "online":
            m_new = torch.maximum(m, s.amax(-1, keepdim=True))
            alpha = ex((m - m_new) * post_t)
            alpha = torch.where(torch.isnan(alpha), torch.zeros_like(alpha), alpha)
            p = ex((s - m_new) * post_t)
        else:
            if kt == 0:
                m_new = rt_ref(m + torch.clamp(s.amax(-1, keepdim=True), min=-30000.0))
            else:
                m_new = m
            p = ex((s - m_new) * post_t + shift)
            over = ~(p.sum(-1, keepdim=True) <= KLIMIT[dtype])
            if bool(over.any()):
                up = torch.clamp((s - m_new).amax(-1, keepdim=True), min=0.0)
                m_new = torch.where(over, rt_ref(m_new + up), m_new)
                p = ex((s - m_new) * post_t + shift)
            alpha = ex(-(m_new - m) * post_t)
            if kt == 0 and mutant != "first_rescale":
                alpha = torch.ones_like(alpha)              # nothing to rescale yet (exp of a far-negative first reference would be inf: 0 inf)
        moved = alpha != 1.0
        if mutant == "skip_rescale" and not skipped and kt > 0 and bool(moved.any()):
            skipped = True                                  # one tile's rescale of O is lost (l still follows)
            o_scaled = o
        else:
            o_scaled = o * alpha
        l = l * alpha + p.sum(-1, keepdim=True)
        m = m_new
        if mutant == "double_key" and mkey // tile == kt:
            l = l + p[:, :, mkey % tile:mkey % tile + 1]
        pk = p if keep is None else torch.where(torch.cat([keep, keep.new_zeros(P, T, Tp - T)], 2)[:, :, sl], p, torch.zeros_like(p))
        if npass == 3:
            ph = rt(pk)
            pl_ = rt(pk - ph)
            o = o_scaled + (ph @ vt[1] + pl_ @ vt[0] + ph @ vt[0])
        else:
            o = o_scaled + rt(pk) @ vt[0]
        if mutant == "double_key" and mkey // tile == kt:
            j = mkey % tile
            o = o + rt(pk[:, :, j:j + 1]) * vt[0][:, j:j + 1]
    res = o * (torch.tensor(inv_keep, dtype=F32) / l)
    if dtype is None:
        return res.double()
    if npass == 3:
        h = rt(res)
        return h.double() + rt(res - h).double()
    return rt_out(res).double()


# ------------------------------------------------------------------------------------------------ the kernels and their cases
# kernel -> (B, T, heads, ch) cases of tests/test_gpu_attn_exact.py (the CPU tier runs the emulation on the same ones)
CASES = {
    "attn_legacy": [(1, 64, 2, 32), (1, 100, 2, 64), (2, 36, 2, 16)],
    "attn64": [(1, 64, 5, 32), (1, 64, 5, 64), (1, 64, 5, 128)],                       # B heads = 5: the second workgroup has three dead waves
    "attn_flash": [(2, 36, 2, 16), (1, 65, 3, 128), (1, 100, 2, 64), (2, 130, 2, 32), (1, 257, 2, 128)],
    "lsa_parity": [(1, 66, 2, 64), (1, 130, 3, 64), (1, 300, 2, 64)],
    "lsa64": [(1, 66, 2, 64), (1, 130, 3, 64), (1, 300, 2, 64)],                       # T = 300: two 256-query blocks, a dead wave
    "lsa_drop": [(1, 130, 2, 64)],
    "lsa_mx8": [(1, 66, 2, 64), (1, 300, 1, 64)],
}


def spec(kernel, precision, ch):
    """(emulate kwargs, bound kwargs, reference function) of a kernel in a precision mode"""
    dt = DTYPES.get(precision)
    if kernel == "attn_legacy":
        pre = float(torch.tensor(1.0, dtype=F32) / torch.sqrt(torch.sqrt(torch.tensor(float(ch), dtype=F32))))
        return dict(form="online", dtype=None, pre=pre), dict(dtype=None), legacy_ref
    if kernel == "attn64":
        post = float(torch.tensor(1.0, dtype=F32) / torch.sqrt(torch.tensor(float(ch), dtype=F32)))
        return dict(form="online", dtype=dt, post=post), dict(dtype=dt), legacy_ref
    if kernel == "attn_flash":
        post = float(torch.tensor(LOG2E, dtype=F32) / torch.sqrt(torch.tensor(float(ch), dtype=F32)))
        return dict(form="mref", dtype=dt, post=post, base2=True, pad="last"), dict(dtype=dt, ref_rounded=True), legacy_ref
    if kernel == "lsa_parity":
        return dict(form="online", dtype=dt, npass=3, base2=True, diag=True), dict(dtype=dt, npass=3), lsa_ref
    if kernel == "lsa64":
        return dict(form="mref", dtype=dt, base2=True, diag=True), dict(dtype=dt, ref_rounded=True), lsa_ref
    if kernel == "lsa_mx8":
        return dict(form="mref", dtype=dt, base2=True, diag=True), dict(dtype=dt, out_dtype=torch.bfloat16), lsa_ref
    raise KeyError(kernel)


def tier2_inputs(kernel, precision, P, T, ch, seed):
    """random operands of a tier-2 case, rounded as the kernel receives them"""
    dt = DTYPES.get(precision)
    if kernel == "attn_legacy":
        return random_qkv(P, T, ch, None, seed, logit_std=1.5)
    if kernel in ("attn64", "attn_flash"):
        return random_qkv(P, T, ch, dt, seed, logit_std=1.5)
    if kernel == "lsa_mx8":
        return mx_quantise(*random_qkv(P, T, ch, None, seed, logit_std=1.5, base2=True))
    return random_qkv(P, T, ch, dt, seed, logit_std=1.5, base2=True, npass=3 if kernel == "lsa_parity" else 1)


def tier2_bound(kernel, precision, r, q, k, v, T, ch):
    _, bk, _ = spec(kernel, precision, ch)
    if bk.get("npass") == 3:
        dt = bk["dtype"]
        lo = tuple(split_lo(x, dt)[1] for x in (q, k, v))
        return bound(r, T, ch, lo=lo, **bk)
    return bound(r, T, ch, **bk)


def mx_one_hot_v(T, ch):
    """v for the e4m3 operand: integers in [-16, 16] (exact in e4m3 under any block scale), two keys differ in some channel unless they
    lie 1023 apart"""
    s_ = torch.arange(T)[:, None]
    c_ = torch.arange(ch)[None, :]
    return torch.where(c_ % 2 == 0, (s_ + 3 * c_) % 33 - 16, (s_ + 5 * c_) % 31 - 15).double()


# ------------------------------------------------------------------------------------------------ Swin-V2 cosine window attention (swin.hip)
# swin_window_attn_kernel: one wave per (window, head). Rounding points: q, k L2-normalised in fp32 (sum of 32 squares: 7 u on the sum,
# 3.5 u after the root, the root itself 2 u, the division 2 u, the product u: NORM_U = 8.5 u relative) and rounded to the operand
# type (three products: to the hi + lo pair, all operands pre-scaled by powers of two); logits = fp32 S scale + rpb (+ -100): e_l =
# (32 + 4) u scale sum |q||k| + 3 u (|logit| + 116); P = exp(. - max) rounded to T (pair), O^T = V^T P, 1 / sum, output rounded to T (pair).
# The single-product reference sees the SAME rounded q, k (swin_operands asserts that no entry lies within NORM_U of a rounding midpoint
# and resamples those that do); the three-product one sees the fp64 normalisation, and 2 (NORM_U + pair) scale sum |q||k| joins e_l.
WS = 8
NORM_U = 8.5 * U
SWIN_CASES = [(16, 16, 0), (9, 17, 4), (4, 4, 4)]          # (H, W, shift); N = 2, heads = 3
SWIN_N, SWIN_HEADS = 2, 3


def swin_index(H, W, shift, roll_delta=0):
    """(ids [nW][64]: source token of every window token, H * W = a pad token; reg [nW][64]: its shift-mask region; masked)"""
    pH, pW = (H + WS - 1) // WS * WS, (W + WS - 1) // WS * WS
    sh, sw = (0 if WS >= pH else shift), (0 if WS >= pW else shift)
    ids = torch.full((pH, pW), H * W, dtype=torch.long)
    ids[:H, :W] = torch.arange(H * W).view(H, W)
    if sh + sw > 0:
        ids = torch.roll(ids, shifts=(-(max(sh - roll_delta, 0) if sh else 0), -(max(sw - roll_delta, 0) if sw else 0)), dims=(0, 1))
    reg = torch.zeros((pH, pW), dtype=torch.long)
    if sh + sw > 0:
        cnt = 0
        for a in ((0, -WS), (-WS, -sh), (-sh, None)):
            for b in ((0, -WS), (-WS, -sw), (-sw, None)):
                reg[a[0]:a[1], b[0]:b[1]] = cnt
                cnt += 1
    part = lambda t: t.view(pH // WS, WS, pW // WS, WS).permute(0, 2, 1, 3).reshape(-1, WS * WS)
    return part(ids), part(reg), sh + sw > 0


def swin_normalize(x):
    """F.normalize(p=2, eps=1e-12) over the last axis, in the dtype of x"""
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def swin_attention(qn, kn, v, pad, scale, rpb, H, W, shift, *, emu=None, roll_delta=0, visible=False):
    """qn, kn, v [N][H*W][heads][32]: normalised (and rounded) q, k and v per token; pad = (q, k, v) [heads][32] of a pad token (the Linear's
    bias, k zero, q normalised); scale [heads]; rpb [heads][64][64]. fp64 reference: dict(out [N][H*W][heads][32], A, w, lmag, vsum, smax).
    emu = (dtype, npass): the fp32 emulation of the kernel instead (returns the stored values as fp64). roll_delta / visible: defects."""
    N, _, heads, _ = qn.shape
    ids, reg, masked = swin_index(H, W, shift, roll_delta)
    nW = ids.shape[0]
    wd = F64 if emu is None else F32
    gather = lambda x, p: torch.cat([x.to(wd), p.to(wd)[None, None].expand(N, 1, heads, 32)], 1)[:, ids].permute(0, 1, 3, 2, 4)   # [N][nW][heads][64][32]
    Q, K, V = gather(qn, pad[0]), gather(kn, pad[1]), gather(v, pad[2])
    bias = rpb.to(wd)[None, None]
    mask = torch.zeros((nW, 1, 64, 64), dtype=wd)
    if masked and not visible:
        mask = torch.where(reg[:, None, :, None] != reg[:, None, None, :], torch.tensor(-100.0, dtype=wd), torch.tensor(0.0, dtype=wd))
    sc = scale.to(wd).view(1, 1, heads, 1, 1)
    res = {}
    if emu is None:
        logit = Q @ K.transpose(-1, -2) * sc + bias + mask[None]
        m = logit.amax(-1, keepdim=True)
        e = torch.exp(logit - m)
        w = e / e.sum(-1, keepdim=True)
        o = w @ V
        vis = (mask[None] == 0).expand_as(logit)
        lo_ = torch.where(vis, logit, m.expand_as(logit)).amin(-1, keepdim=True)
        res = dict(A=w @ V.abs(), vsum=V.abs().sum(-2, keepdim=True).expand_as(o), wv=w,
                   lmag=((Q.abs() @ K.abs().transpose(-1, -2)) * sc).amax(-1, keepdim=True).expand(*o.shape[:-1], 1),
                   smax=(logit.abs() + 116.0).amax(-1, keepdim=True).expand(*o.shape[:-1], 1), spread=float((m - lo_).max()) * LOG2E, unit=LOG2E)
    else:
        dtype, npass = emu
        rt = lambda x: x.to(dtype).to(F32)
        if npass == 3:
            Qs, Ks, Vs = Q * 64.0, K * 64.0, V * 64.0
            Qh, Kh, Vh = rt(Qs), rt(Ks), rt(Vs)
            Ql, Kl, Vl = rt(Qs - Qh), rt(Ks - Kh), rt(Vs - Vh)
            S = Kh @ Qh.transpose(-1, -2) + Kh @ Ql.transpose(-1, -2) + Kl @ Qh.transpose(-1, -2)
            logit = S.transpose(-1, -2) * (sc * torch.tensor(1.0 / 4096.0, dtype=F32)) + bias
        else:
            Qh, Kh, Vh = rt(Q), rt(K), rt(V)
            logit = (Qh @ Kh.transpose(-1, -2)) * sc + bias
        logit = torch.where(mask[None] != 0, logit + torch.tensor(-100.0, dtype=F32), logit)
        p = torch.exp2((logit - logit.amax(-1, keepdim=True)) * torch.tensor(LOG2E, dtype=F32))
        l = p.sum(-1, keepdim=True)
        if npass == 3:
            ps = p * 1024.0
            ph = rt(ps)
            pl_ = rt(ps - ph)
            o = (ph @ Vh + pl_ @ Vh + ph @ Vl) * (1.0 / (l * 65536.0))
            o = rt(o).double() + rt(o - rt(o)).double()
        else:
            o = rt((rt(p) @ Vh) * (1.0 / l)).double()
    # every token's row goes back to its own place; pad tokens are not stored
    def scatter(x):
        x = x.permute(0, 1, 3, 2, 4).reshape(N, nW * 64, heads, x.shape[-1])
        out = x.new_zeros((N, H * W + 1, heads, x.shape[-1]))
        out[:, ids.reshape(-1)] = x
        return out[:, :H * W]
    if emu is not None:
        return scatter(o)
    out = {k_: (scatter(x) if torch.is_tensor(x) and x.dim() == 5 and x.shape[-1] in (1, 32) else x) for k_, x in res.items() if k_ != "wv"}
    out["out"] = scatter(o)
    out["wv"], out["ids"] = res["wv"], ids
    return out


def swin_bound(r, dtype, npass):
    """the per-element bound of a swin_attention reference r (module comment above). Three products: the dropped lo.lo terms are
    u_T^2 lmag in the logits and u_T^2 A in the output (|lo| <= u_T |hi|), v's pair misses the fp32 value by `pair`."""
    uT, fl = u_of(dtype)
    out, A = r["out"].abs(), r["A"]
    e_l = (32 + 4) * U * r["lmag"] + 3 * U * r["smax"]
    if npass == 3:
        pair = plane_terms(dtype)[0]
        e_l = e_l + 2 * (NORM_U + pair) * r["lmag"] + uT * uT * r["lmag"]
    e_p = torch.expm1(e_l) + U * (r["smax"] + 1.0) + 2 * U
    b = 2 * e_p * A + (64 + 8) * U * (A + out)
    if npass == 3:
        b = b + (2 * uT * uT + pair + uT * uT) * A + 2 * uT * uT * (out + b) + fl
        return b
    b = b + uT * A + fl * r["vsum"]
    return b + uT * (out + b) + fl


def _ulp16(x, dtype):
    bits, emin = (10, -24) if dtype == torch.float16 else (7, -133)
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -140)))
    return torch.exp2(torch.clamp(e - bits, min=emin))


def swin_operands(N, H, W, heads, dtype, npass, seed, in16=False):
    """random qkv rows [N*H*W][3 * heads * 32] (fp32 values; in16: already rounded to dtype), the Linear's bias with the k third zero, and
    the operands the kernel must end up with: (qn, kn, v) [N][H*W][heads][32] and the pad token's. Single product: no normalised entry
    lies within NORM_U of a rounding midpoint of dtype (rows that do are resampled), so the fp32 normalisation rounds as the fp64 one."""
    g = _gen(seed)
    C = heads * 32
    rows = N * H * W
    rnd_in = (lambda x: x.to(dtype).float()) if in16 else (lambda x: x)
    qkv = rnd_in(torch.randn(rows, 3, heads, 32, generator=g))
    bias = torch.randn(3, heads, 32, generator=g) * 0.5
    bias[1] = 0.0

    def settle(x):                      # x [..., 32] fp32 -> resample rows until every normalised entry is clear of a midpoint
        for _ in range(200):
            n64 = swin_normalize(x.double())
            r16 = n64.to(dtype).double()
            room = _ulp16(r16, dtype) / 2 - (n64 - r16).abs()
            bad = (room <= NORM_U * n64.abs() + 2.0 ** -149).any(-1)
            if not bool(bad.any()):
                return x
            x = x.clone()
            x[bad] = rnd_in(torch.randn(int(bad.sum()), 32, generator=g))
        raise AssertionError("midpoints")
    if npass == 1:
        qkv[:, 0] = settle(qkv[:, 0])
        qkv[:, 1] = settle(qkv[:, 1])
        bias[0] = settle(bias[0])
    rq = (lambda x: x.to(dtype).double()) if npass == 1 else (lambda x: x)
    x64 = qkv.double().view(N, H * W, 3, heads, 32)
    qn, kn = rq(swin_normalize(x64[:, :, 0])), rq(swin_normalize(x64[:, :, 1]))
    if npass == 1:
        v = x64[:, :, 2].to(dtype).double()
        pad = (rq(swin_normalize(bias[0].double())), torch.zeros(heads, 32, dtype=F64), bias[2].double().to(dtype).double())
    else:
        v = x64[:, :, 2]
        pad = (swin_normalize(bias[0].double()), torch.zeros(heads, 32, dtype=F64), bias[2].double())
    return qkv.reshape(rows, 3 * C).contiguous(), bias.reshape(3 * C).contiguous(), (qn, kn, v), pad


def swin_uniform(N, H, W, heads):
    """tier 1: q third zero (cosine logits 0), rpb 0; the channels of v hold the bits of the source token's (y, x, sample) as 0 / 1, in another
    channel order per head; the pad token's v is 0.5 on the even channels. Returns (qkv rows fp32, bias, (qn, kn, v), pad)."""
    C = heads * 32
    t = torch.arange(N * H * W)
    n, y, x = t // (H * W), (t // W) % H, t % W
    code = (y | (x << 5) | (n << 10))[:, None, None]
    c = (torch.arange(32)[None, None, :] + 5 * torch.arange(heads)[None, :, None]) % 32
    v = ((code >> (c % 11)) & 1).double() * torch.where(c < 22, 1.0, 0.5).double()
    g = _gen(1)
    k = (torch.randn(N * H * W, heads, 32, generator=g) * 8).round().double() / 8          # exact in f16 and bf16
    qkv = torch.stack([torch.zeros_like(v), k, v], 1)                    # [rows][3][heads][32]
    bias = torch.zeros(3, heads, 32, dtype=F64)
    bias[2, :, 0::2] = 0.5
    ops_ = (torch.zeros(N, H * W, heads, 32, dtype=F64), swin_normalize(k).view(N, H * W, heads, 32), v.view(N, H * W, heads, 32))
    pad = (torch.zeros(heads, 32, dtype=F64), torch.zeros(heads, 32, dtype=F64), bias[2])
    return qkv.float().reshape(-1, 3 * C).contiguous(), bias.float().reshape(3 * C).contiguous(), ops_, pad
