"""Plain-torch restatement of the set-ViT style encoder (networks/vit_set.py) and of its backward, layer by layer with explicit formulas (no
autograd in `backward`). `forward` is differentiable, so the same function serves as the autograd reference (fp32 against fp64: the bound of
the CPU tier; with `rnd`: the operand-rounding figure that bounds the GPU tier). The building blocks (`ln_bwd`, `gelu_grad`, `lsa_bwd`,
`head_bwd`, `tok_bwd`, `patch_rows`) are what the kernels of csrc/svit_bwd.hip implement.

P: parameters under the reference's state-dict names. cfg: dict(patch, heads, pool, p_emb, p_drop). keeps: {site: bool tensor} from
oracle/dropmask.py (site ids of stedm_amd.style.sViT), or None where p == 0."""
import math

import numpy as np
import torch

SITE_EMB, SITE_ATTN, SITE_OUT, SITE_FF1, SITE_FF2 = 0x10000, 1, 2, 3, 4
EPS = 1e-5


def depth_of(P) -> int:
    return 1 + max(int(k.split(".")[2]) for k in P if k.startswith("transformer.layers."))


def patch_rows(img: torch.Tensor, p: int) -> torch.Tensor:
    """[B, ns, H, W, 3] -> [B, n, p*p*3*ns]: channel-stack the set (channel = c * ns + s, vit_set.py:105-106), 'b c (h p1) (w p2) -> b (h w) (p1 p2 c)'."""
    B, ns, H, W, _ = img.shape
    x = img.permute(0, 4, 1, 2, 3).reshape(B, 3 * ns, H, W)
    hp, wp = H // p, W // p
    return x.reshape(B, 3 * ns, hp, p, wp, p).permute(0, 2, 4, 3, 5, 1).reshape(B, hp * wp, p * p * 3 * ns)


def make_keeps(B: int, T: int, dim: int, mlp: int, heads: int, depth: int, p_emb: float, p_drop: float, seed: int):
    from oracle import dropmask
    keeps = {}
    el = lambda shape, p, site: torch.from_numpy(dropmask.keep_elementwise(int(np.prod(shape)), p, seed, site).reshape(shape).copy())
    if p_emb > 0:
        keeps[SITE_EMB] = el((B, T, dim), p_emb, SITE_EMB)
    if p_drop > 0:
        for l in range(depth):
            keeps[8 * l + SITE_ATTN] = torch.from_numpy(dropmask.keep_attention(B * heads, T, p_drop, seed, 8 * l + SITE_ATTN).reshape(B, heads, T, T).copy())
            keeps[8 * l + SITE_OUT] = el((B, T, dim), p_drop, 8 * l + SITE_OUT)
            keeps[8 * l + SITE_FF1] = el((B, T, mlp), p_drop, 8 * l + SITE_FF1)
            keeps[8 * l + SITE_FF2] = el((B, T, dim), p_drop, 8 * l + SITE_FF2)
    return keeps


def _drop(x, keeps, site, p):
    if p <= 0:
        return x
    return x * (keeps[site].to(x.dtype) / (1.0 - p))


def _ln(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + EPS) * w + b


def rounder(mode: str):
    """Operand rounding of a precision mode, straight-through for autograd: 'f16' / 'bf16' one 16-bit value, 'parity' fp16 hi + lo."""
    def r(x):
        if mode == "f16":
            y = x.detach().float().half().to(x.dtype)
        elif mode == "bf16":
            y = x.detach().float().bfloat16().to(x.dtype)
        elif mode == "parity":
            xf = x.detach().float()
            hi = xf.half().float()
            y = (hi + (xf - hi).half().float()).to(x.dtype)
        else:
            raise ValueError(mode)
        return x + (y - x.detach())
    return r


def forward(P, img, cfg, keeps, rnd=None):
    """-> (out [B, num_classes], tape). rnd: operand rounding applied to both operands of every Linear and of the two attention products."""
    r = rnd if rnd is not None else (lambda t: t)
    lin = lambda x, w, b=None: r(x) @ r(w).transpose(-1, -2) + (0 if b is None else b)
    p, heads, p_emb, p_drop = cfg["patch"], cfg["heads"], cfg["p_emb"], cfg["p_drop"]
    tape = {}
    rows = patch_rows(img, p)
    B, n, _ = rows.shape
    pre = "to_patch_embedding.to_patch_tokens."
    peln = _ln(rows, P[pre + "1.weight"], P[pre + "1.bias"])
    tok = lin(peln, P[pre + "2.weight"], P[pre + "2.bias"])
    dim = tok.shape[-1]
    x = torch.cat((P["cls_token"].expand(B, 1, dim), torch.zeros(B, 1, dim, dtype=tok.dtype), tok), dim=1) + P["pos_embedding"][:, :n + 2]
    x = _drop(x, keeps, SITE_EMB, p_emb)
    tape.update(rows=rows, peln=peln)
    T = n + 2
    eye = torch.eye(T, dtype=torch.bool)
    for l in range(depth_of(P)):
        a, f = f"transformer.layers.{l}.0.", f"transformer.layers.{l}.1."
        ln0 = _ln(x, P[a + "norm.weight"], P[a + "norm.bias"])
        qkv = lin(ln0, P[a + "fn.to_qkv.weight"])
        q, k, v = (t.reshape(B, T, heads, 64).permute(0, 2, 1, 3) for t in qkv.chunk(3, dim=-1))
        scale = P[a + "fn.temperature"].exp()
        dots = (r(q * scale) @ r(k).transpose(-1, -2))
        dots = dots.masked_fill(eye, -torch.finfo(dots.dtype).max)
        prob = dots.softmax(-1)
        pd = _drop(prob, keeps, 8 * l + SITE_ATTN, p_drop)
        att = (r(pd) @ r(v)).permute(0, 2, 1, 3).reshape(B, T, heads * 64)
        y = lin(att, P[a + "fn.to_out.0.weight"], P[a + "fn.to_out.0.bias"])
        tape[f"a{l}"] = dict(x=x, ln=ln0, q=q, k=k, v=v, prob=prob, att=att)
        x = _drop(y, keeps, 8 * l + SITE_OUT, p_drop) + x
        ln1 = _ln(x, P[f + "norm.weight"], P[f + "norm.bias"])
        hpre = lin(ln1, P[f + "fn.net.0.weight"], P[f + "fn.net.0.bias"])
        h = 0.5 * hpre * (1.0 + torch.erf(hpre / math.sqrt(2.0)))
        hd = _drop(h, keeps, 8 * l + SITE_FF1, p_drop)
        y = lin(hd, P[f + "fn.net.3.weight"], P[f + "fn.net.3.bias"])
        tape[f"f{l}"] = dict(x=x, ln=ln1, pre=hpre, hd=hd)
        x = _drop(y, keeps, 8 * l + SITE_FF2, p_drop) + x
    pooled = x.mean(dim=1) if cfg["pool"] == "mean" else x[:, 0]
    z = _ln(pooled, P["mlp_head.0.weight"], P["mlp_head.0.bias"])
    out = lin(z, P["mlp_head.1.weight"], P["mlp_head.1.bias"])
    tape.update(x_out=x, pooled=pooled, z=z)
    return out, tape


# ---------------------------------------------------------------------------------------------------- explicit backward pieces
def ln_bwd(x, dy, gamma):
    """-> dx, dgamma, dbeta (stedm_ln_bwd): xh = (x - mean) rstd, dxh = dy gamma, dx = rstd (dxh - mean(dxh) - xh mean(dxh xh))."""
    mu = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + EPS)
    xh = (x - mu) * rstd
    dxh = dy * gamma
    dx = rstd * (dxh - dxh.mean(-1, keepdim=True) - xh * (dxh * xh).mean(-1, keepdim=True))
    red = tuple(range(x.dim() - 1))
    return dx, (dy * xh).sum(red), dy.sum(red)


def gelu_grad(pre):
    """gelu'(x) of the exact erf GELU: Phi(x) + x phi(x)."""
    return 0.5 * (1.0 + torch.erf(pre / math.sqrt(2.0))) + pre * torch.exp(-0.5 * pre * pre) / math.sqrt(2.0 * math.pi)


def lsa_bwd(q, k, v, temperature, d_att, keep=None, p: float = 0.0):
    """q, k, v [B, h, T, 64] (unscaled q), d_att [B, h, T, 64] -> dq, dk, dv, d_temperature (stedm_lsa_bwd):
         dots = q k^T exp(temperature), diagonal masked (its probability is exactly 0), P = softmax(dots), Pd = P keep / (1 - p)
         dPd = d_att v^T;  dv = Pd^T d_att;  D = rowsum(Pd o dPd) (= rowsum(d_att o O))
         dS = P o (keep / (1 - p) dPd - D)   (0 on the masked diagonal)
         dq = dS k exp(temperature);  dk = dS^T q exp(temperature);  d_temperature = sum dS o dots."""
    T = q.shape[-2]
    scale = temperature.exp()
    raw = (q * scale) @ k.transpose(-1, -2)
    eye = torch.eye(T, dtype=torch.bool)
    prob = raw.masked_fill(eye, -torch.finfo(raw.dtype).max).softmax(-1)
    assert float(prob.diagonal(dim1=-2, dim2=-1).abs().max()) == 0.0       # the masked diagonal contributes nothing
    ks = torch.ones_like(prob) if keep is None or p <= 0 else keep.to(prob.dtype) / (1.0 - p)
    pd = prob * ks
    dpd = d_att @ v.transpose(-1, -2)
    dv = pd.transpose(-1, -2) @ d_att
    D = (pd * dpd).sum(-1, keepdim=True)
    dS = prob * (ks * dpd - D)
    dq = dS @ k * scale
    dk = dS.transpose(-1, -2) @ q * scale
    dtemp = (dS * raw).sum()
    return dq, dk, dv, dtemp


def head_bwd(x, pool: str, ln_w, ln_b, w, d_out):
    """-> dx [B, T, dim], d ln_w, d ln_b, d w, d bias (stedm_svit_head_bwd); b-sums in ascending order."""
    B, T, dim = x.shape
    pooled = x.mean(dim=1) if pool == "mean" else x[:, 0]
    mu = pooled.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((pooled - mu) ** 2).mean(-1, keepdim=True) + EPS)
    xh = (pooled - mu) * rstd
    dz = d_out @ w
    dpool, dg, db = ln_bwd(pooled, dz, ln_w)
    dx = dpool[:, None, :].expand(B, T, dim) / T if pool == "mean" else torch.cat((dpool[:, None, :], torch.zeros(B, T - 1, dim, dtype=x.dtype)), dim=1)
    return dx.contiguous(), dg, db, d_out.transpose(0, 1) @ (xh * ln_w + ln_b), d_out.sum(0)


def tok_bwd(dx):
    """svit_tok_place reversed -> d pos [T, dim], d cls [dim], d tok [B * (T - 2), dim]; batch sums in ascending b."""
    B, T, dim = dx.shape
    dpos = torch.zeros(T, dim, dtype=dx.dtype)
    for b in range(B):
        dpos = dpos + dx[b]
    return dpos, dpos[0].clone(), dx[:, 2:].reshape(B * (T - 2), dim).clone()


def backward(P, tape, g, cfg, keeps):
    """Gradients of (out * g).sum() for every parameter of P, by the explicit formulas; no autograd."""
    heads, p_emb, p_drop = cfg["heads"], cfg["p_emb"], cfg["p_drop"]
    ks = lambda site, p: 1.0 if p <= 0 else keeps[site].to(g.dtype) / (1.0 - p)
    G = {}
    x_out = tape["x_out"]
    B, T, dim = x_out.shape
    # head: out = LN(pool(x)) W^T + b
    G["mlp_head.1.weight"] = g.transpose(0, 1) @ tape["z"]
    G["mlp_head.1.bias"] = g.sum(0)
    dpool, G["mlp_head.0.weight"], G["mlp_head.0.bias"] = ln_bwd(tape["pooled"], g @ P["mlp_head.1.weight"], P["mlp_head.0.weight"])
    if cfg["pool"] == "mean":
        dx = (dpool[:, None, :] / T).expand(B, T, dim).clone()
    else:
        dx = torch.zeros_like(x_out)
        dx[:, 0] = dpool
    flat = lambda t: t.reshape(-1, t.shape[-1])
    for l in reversed(range(depth_of(P))):
        a, f = f"transformer.layers.{l}.0.", f"transformer.layers.{l}.1."
        # FeedForward: x_out = drop(W2 drop(gelu(W1 LN(x) + b1)) + b2) + x
        t = tape[f"f{l}"]
        dy = dx * ks(8 * l + SITE_FF2, p_drop)
        G[f + "fn.net.3.bias"] = flat(dy).sum(0)
        G[f + "fn.net.3.weight"] = flat(dy).transpose(0, 1) @ flat(t["hd"])
        dh = (dy @ P[f + "fn.net.3.weight"]) * ks(8 * l + SITE_FF1, p_drop)
        dpre = dh * gelu_grad(t["pre"])
        G[f + "fn.net.0.bias"] = flat(dpre).sum(0)
        G[f + "fn.net.0.weight"] = flat(dpre).transpose(0, 1) @ flat(t["ln"])
        dxn, G[f + "norm.weight"], G[f + "norm.bias"] = ln_bwd(t["x"], dpre @ P[f + "fn.net.0.weight"], P[f + "norm.weight"])
        dx = dx + dxn
        # LSA: x_out = drop(Wo attention(Wqkv LN(x)) + bo) + x
        t = tape[f"a{l}"]
        dy = dx * ks(8 * l + SITE_OUT, p_drop)
        G[a + "fn.to_out.0.bias"] = flat(dy).sum(0)
        G[a + "fn.to_out.0.weight"] = flat(dy).transpose(0, 1) @ flat(t["att"])
        datt = (dy @ P[a + "fn.to_out.0.weight"]).reshape(B, T, heads, 64).permute(0, 2, 1, 3)
        dq, dk, dv, dtemp = lsa_bwd(t["q"], t["k"], t["v"], P[a + "fn.temperature"], datt, keeps.get(8 * l + SITE_ATTN), p_drop)
        G[a + "fn.temperature"] = dtemp
        dqkv = torch.cat([u.permute(0, 2, 1, 3).reshape(B, T, heads * 64) for u in (dq, dk, dv)], dim=-1)
        G[a + "fn.to_qkv.weight"] = flat(dqkv).transpose(0, 1) @ flat(t["ln"])
        dxn, G[a + "norm.weight"], G[a + "norm.bias"] = ln_bwd(t["x"], dqkv @ P[a + "fn.to_qkv.weight"], P[a + "norm.weight"])
        dx = dx + dxn
    # embedding: x = drop(cat(cls, 0, tok) + pos)
    dxe = dx * ks(SITE_EMB, p_emb)
    G["pos_embedding"] = dxe.sum(0, keepdim=True)
    G["cls_token"] = dxe[:, 0].sum(0).reshape(1, 1, dim)
    dtok = dxe[:, 2:]
    pre = "to_patch_embedding.to_patch_tokens."
    G[pre + "2.bias"] = flat(dtok).sum(0)
    G[pre + "2.weight"] = flat(dtok).transpose(0, 1) @ flat(tape["peln"])
    _, G[pre + "1.weight"], G[pre + "1.bias"] = ln_bwd(tape["rows"], dtok @ P[pre + "2.weight"], P[pre + "1.weight"])
    for k in ("to_time_embedding.weight", "to_time_embedding.bias"):
        if k in P:
            G[k] = torch.zeros_like(P[k])        # t_emb is always None: no gradient reaches it
    return G


def autograd_grads(P, img, g, cfg, keeps, dtype=torch.float32, rnd=None):
    """Gradients of (forward(...) * g).sum() by torch autograd in `dtype` -> (out, {name: grad})."""
    Pd = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in P.items()}
    with torch.enable_grad():
        out, _ = forward(Pd, img.to(dtype), cfg, keeps, rnd=rnd)
        (out * g.to(dtype)).sum().backward()
    return out.detach(), {k: (torch.zeros_like(v) if v.grad is None else v.grad.detach()) for k, v in Pd.items()}


def rel_err(a, ref) -> float:
    """max-abs error over max-abs reference (the metric of every bound of this feature)."""
    den = float(ref.abs().max())
    return float((a.double() - ref.double()).abs().max()) / den if den > 0 else float((a.double() - ref.double()).abs().max())
