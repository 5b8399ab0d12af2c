"""CPU tier: a masked DDIM loop (ddim.py:113-162 with the blend of :143-146) assembled here from the oracle's pieces (oracle/ddim.py:
DDIMSchedule, cfg_combine, ddim_update, q_sample), pinned against F17 (tests/golden/make_golden_mask.py: the reference's own DDIMSampler
with recorded noises). The GPU tier (tests/test_gpu_masked_sampler.py) checks the HIP sampler against this loop."""
import numpy as np
import torch

from oracle import ddim as oddim

torch.set_grad_enabled(False)


@torch.no_grad()
def masked_ddim_sample(apply_model, sched, x_T, cond, S, mask, x0, q_noises, eta=0.0, uncond=None, scale=1.0, noises=None,
                       log_every_t=100, rescale_phi=0.7):
    """The reference's masked loop: at iteration i (index = total - i - 1, t = timesteps[index]) img = q_sample(x0, t, q_noises[i]) * mask
    + (1 - mask) * img before the model call; then the DDIM step (noise `noises[i]`, None: sigma * noise == 0). Returns
    (img, x_inter), x_inter logging the unblended img as ddim.py:158-160 does (initial entry: x_T)."""
    ds = oddim.DDIMSchedule(sched, S, eta)
    ts = ds.ddim_timesteps
    total = ts.shape[0]
    img = x_T
    b = x_T.shape[0]
    x_inter = [img]
    for i, step in enumerate(np.flip(ts)):
        index = total - i - 1
        t = torch.full((b,), int(step), dtype=torch.long)
        img = oddim.q_sample(sched, x0, t, q_noises[i]) * mask + (1.0 - mask) * img
        if uncond is None or scale == 1.0:
            e_t = apply_model(img, t, cond)
        else:
            e_t = oddim.cfg_combine(apply_model(img, t, cond), apply_model(img, t, uncond), scale, rescale_phi)
        img, _ = oddim.ddim_update(img, e_t, *ds.scalars(index), None if noises is None else noises[i])
        if index % log_every_t == 0 or index == total - 1:
            x_inter.append(img)
    return img, x_inter


def toy_eps(x, t, c):
    """the closed-form eps model of F10 / F17 (make_golden.py, make_golden_mask.py)"""
    tf = t.float()[:, None, None, None] / 1000.0
    return torch.tanh(x * (0.5 + tf) + c["bias"]) * (0.8 + 0.3 * tf) + 0.1 * c["bias"]


def f17_case(fx, case):
    """the inputs of F17 case 'a' or 'b' as keyword arguments of masked_ddim_sample (CPU tensors)"""
    T = lambda k: torch.from_numpy(np.asarray(fx[k]))
    kw = dict(x_T=T("xT"), cond={"bias": T("cond")}, mask=T(f"{case}_mask"), x0=T("x0"), q_noises=list(T(f"{case}_q_noises")))
    if case == "a":
        kw.update(S=20, eta=0.0, uncond={"bias": T("uncond")}, scale=1.5, log_every_t=5)
    else:
        kw.update(S=10, eta=1.0, noises=list(T("b_step_noises")))
    return kw


def rel(a, b):
    a, b = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.std())


def test_f17_masked_loop_matches_the_reference_sampler(golden):
    fx = golden("f17_ddim_mask")
    sched = oddim.Schedule()
    for case in ("a", "b"):
        calls = [0]

        def am(x, t, c):
            calls[0] += 1
            return toy_eps(x, t, c)

        out, x_inter = masked_ddim_sample(am, sched, **f17_case(fx, case))
        assert calls[0] == int(fx[f"{case}_calls"])
        err = rel(out, fx[f"{case}_out"])
        assert err < 1e-5, (case, err)
        if case == "a":
            assert len(x_inter) == 6
            assert rel(torch.stack(x_inter), fx["a_x_inter"]) < 1e-5
            assert torch.equal(x_inter[0], torch.from_numpy(fx["xT"]))       # logged before the first blend


def test_f17_mask_extremes_behave_as_the_semantics_say(golden):
    """mask == 0 is the unmasked sampler; the kept region of mask == 1 ends close to x0 (the last step's output, not x0 itself)."""
    fx = golden("f17_ddim_mask")
    sched = oddim.Schedule()
    kw = f17_case(fx, "a")
    zero = torch.zeros_like(kw["mask"])
    out0, _ = masked_ddim_sample(toy_eps, sched, **dict(kw, mask=zero))
    plain = oddim.ddim_sample(toy_eps, sched, kw["x_T"], kw["cond"], 20, 0.0, uncond=kw["uncond"], scale=1.5)
    assert torch.equal(out0, plain)
    out1, _ = masked_ddim_sample(toy_eps, sched, **dict(kw, mask=torch.ones_like(kw["mask"])))
    x0 = kw["x0"]
    assert not torch.equal(out1, x0)
    assert float((out1 - x0).abs().max()) < 0.5 * float(x0.std())
