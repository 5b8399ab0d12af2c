"""fp64 restatement of the training objective the loss kernel computes (stedm_amd/csrc/bwd.hip: stedm_diffusion_loss; the reference's
p_losses, ddpm.py:1015-1048 with get_loss :282-295), written from the formulas of include/stedm_hip.h, and the error bounds that go with
it. Shared by tests/test_objective_cpu.py (pins this file against the reference's own p_losses + autograd, fixture F24) and
tests/test_gpu_objective.py (pins the kernel and the training step against this file).

    ls_b   = mean_i f(target - pred)                 f = |.| (kind 0) or (.)^2 (kind 1)        lv_b = logvar[t_b]
    gamma  = mean_b(ls_b exp(-lv_b) + lv_b)          vlb = mean_b(lvlb[t_b] ls_b)              simple = mean_b ls_b
    loss   = lsw gamma + ew vlb
    c_b    = (lsw exp(-lv_b) + ew lvlb[t_b]) gscale / (B n)                                    d_pred[b, i] = c_b f'(pred - target)
    d_logvar[k] = lsw gscale / B sum_{b: t_b = k} (1 - ls_b exp(-logvar[k]))

Bounds count fp32 roundings (U = 2^-24 per correctly rounded operation, 2U for an exp), each acting on the magnitude of what it rounds:
a sum of terms of both signs is bounded against the sum of their magnitudes.
  * the kernel forms every sum in fp64 and narrows each result once: K_KERNEL = 2 for a scalar or a d_logvar entry (the narrowing, and one more
    U that covers the fp64 work: n + B additions and an exp at 2^-53 each, below U for any n + B < 2^28). A d_pred element is c_b (narrowed: 1)
    times 2 d (l2: the fp32 difference rounds: 1, the doubling is exact) rounded once more (1): K_KERNEL_DPRED = 4 with the fp64 allowance; on
    dyadic inputs the difference is exact and the count is still an upper bound.
  * the reference runs p_losses and its autograd graph in fp32. Forward, per sample: difference (1), square (1; abs: 0), a sum of n terms
    (<= n - 1 in any order), the division by n (1) -> n + 2; then exp (2), quotient (1), + lv (1), the batch sum (B - 1) and division (1), the
    products with lvlb, l_simple_weight and original_elbo_weight (3) and the final sum (1): K_REF = n + B + 11, taken as n + B + 12.
    Backward to model_output, per path (the simple and the vlb path each call get_loss): weight (1), / B (1), exp (2) and quotient (1) or
    lvlb (1), / n (1), the difference (1), the product (1) -> at most 8; the two paths add (1): 9 <= K_REF_DPRED = 12.
F24 (reference against fp64, and reference against kernel) is held to the reference's count plus the kernel's."""
import torch

U = 2.0 ** -24
K_KERNEL = 2
K_KERNEL_DPRED = 4
K_REF_DPRED = 12


def k_ref(n: int, B: int) -> int:
    return n + B + 12


def objective(pred, target, t, logvar, lvlb, kind, lsw=1.0, ew=0.0, gscale=1.0):
    """All of the kernel's outputs in fp64 (inputs of any float dtype, on any device) plus the magnitudes the bounds act on.
    -> dict: loss, loss_simple, loss_gamma, loss_vlb (0-dim), ls [B], c [B], d_pred (like pred), d_logvar [T], and mag_* (see bounds)."""
    p, q = pred.double(), target.double()
    B = p.shape[0]
    n = p.numel() // B
    d = (p - q).reshape(B, n)
    ls = (d.abs() if kind == 0 else d * d).sum(1) / n
    lv_all = logvar.double()
    lv, w = lv_all[t], lvlb.double()[t]
    e = torch.exp(-lv)
    gamma_b = ls * e + lv
    r = {"ls": ls, "loss_simple": ls.mean(), "loss_gamma": gamma_b.mean(), "loss_vlb": (w * ls).mean()}
    r["loss"] = lsw * r["loss_gamma"] + ew * r["loss_vlb"]
    r["c"] = (lsw * e + ew * w) * gscale / (B * n)
    fp = torch.sign(d) if kind == 0 else 2.0 * d
    r["d_pred"] = (r["c"][:, None] * fp).reshape(pred.shape)
    dl = torch.zeros_like(lv_all)
    mag_dl = torch.zeros_like(lv_all)
    for b in range(B):                      # index order, as the kernel
        k = int(t[b])
        dl[k] += 1.0 - ls[b] * e[b]
        mag_dl[k] += 1.0 + ls[b] * e[b]
    r["d_logvar"] = lsw * gscale / B * dl
    r["mag_d_logvar"] = abs(lsw * gscale) / B * mag_dl
    r["mag_loss_simple"] = r["loss_simple"]
    r["mag_loss_gamma"] = (ls * e + lv.abs()).mean()
    r["mag_loss_vlb"] = r["loss_vlb"].abs()
    r["mag_loss"] = abs(lsw) * r["mag_loss_gamma"] + abs(ew) * r["mag_loss_vlb"]
    return r


SCALARS = ("loss", "loss_simple", "loss_gamma", "loss_vlb")


def scalar_bound(r, name, K):
    return K * U * float(r["mag_" + name])


def d_pred_bound(r, K):
    return K * U * r["d_pred"].abs()


def d_logvar_bound(r, K):
    return K * U * r["mag_d_logvar"]


def unet_objective_and_grads(P, cfg, x, t, ctx, target, logvar, lvlb, kind, lsw, ew):
    """The objective over oracle/unet.py's forward, reverse-mode gradients by autograd (the counterpart of oracle.train.unet_loss_and_grads
    for the full objective). Runs in the dtype of its inputs. -> (loss, {param name: grad}, dL/dx, dL/dcontext, model output)"""
    from oracle import unet as ounet
    Pg = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    xg = x.detach().clone().requires_grad_(True)
    cg = ctx.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        y = ounet.unet_forward.__wrapped__(Pg, cfg, xg, t, cg)
        d = target - y
        ls = (d.abs() if kind == 0 else d * d).mean(dim=[1, 2, 3])
        lv = logvar.to(y.dtype)[t]
        loss = lsw * (ls / torch.exp(lv) + lv).mean() + ew * (lvlb.to(y.dtype)[t] * ls).mean()
        loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in Pg.items()}, xg.grad, cg.grad, y.detach()
