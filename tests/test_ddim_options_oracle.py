"""CPU tier: DDIM with temperature, noise_dropout and quantize_x0 (ddim.py:201-210). A loop assembled here from the oracle's pieces
(oracle/ddim.py) plus the three options is pinned against F21 (tests/golden/make_golden_ddim_opts.py: the reference's own DDIMSampler with
recorded noises and dropout masks); the keep rule of the HIP kernel (include/stedm_hip.h, stedm_ddim_step_ex) is restated in numpy; the
sampler's option handling is checked without a GPU (refusals before any device work, eta == 0 keeps the plain step, the options reach the
kernels). The GPU tier (tests/test_gpu_ddim_options.py) checks the kernels and the HIP sampler against these restatements."""
import numpy as np
import pytest
import torch

from oracle import ddim as oddim
from oracle.dropmask import philox4x32_10
from stedm_amd.utils import prng

torch.set_grad_enabled(False)
F21_SEED, F21_S = 21, 10
F21_CASES = {"a": dict(eta=1.0, temperature=0.7), "b": dict(eta=0.5, noise_dropout=0.2), "c": dict(eta=0.0, quantize_x0=True),
             "d": dict(eta=1.0, temperature=0.7, noise_dropout=0.2, quantize_x0=True, cfg=1.5)}


# ------------------------------------------------------------------------------------------------ restatements
def keep_mask(seed: int, sample_ids, n: int, iteration: int, p: float) -> np.ndarray:
    """bool [len(ids), n]: the noise-dropout keep bits of stedm_ddim_step_ex. Element e of sample sid keeps iff u16 >= lrint(p * 65536),
    u16 = field (e & 7) (half (j & 1) of output word j >> 1) of Philox4x32-10(counter {e >> 3, 0x20000 + iteration, 0x44524F50, 0},
    key {seed & 0xFFFFFFFF, sid})."""
    thr = int(np.rint(float(np.float32(p)) * 65536.0))
    g = np.arange((n + 7) // 8, dtype=np.uint64)
    rows = []
    for sid in sample_ids:
        r = philox4x32_10(g, np.uint64(0x20000 + iteration), np.uint64(0x44524F50), np.uint64(0), seed & 0xFFFFFFFF, int(sid) & 0xFFFFFFFF)
        u = np.empty((len(g), 8), dtype=np.uint32)
        for j in range(8):
            u[:, j] = (r[j >> 1] >> np.uint32(16 * (j & 1))) & np.uint32(0xFFFF)
        rows.append(u.reshape(-1)[:n] >= thr)
    return np.stack(rows)


def drop_scale(p: float) -> float:
    """(float)(1 / (1 - p)) with p as the float the C ABI receives."""
    return float(np.float32(1.0 / (1.0 - float(np.float32(p)))))


def vq_quantize(z: torch.Tensor, emb: torch.Tensor) -> torch.Tensor:
    """VectorQuantizer2's eval path (make_golden_ddim_opts.vq_quantize): the straight-through value z + (e_idx - z)."""
    zp = z.permute(0, 2, 3, 1).contiguous()
    zf = zp.view(-1, emb.shape[1])
    d = torch.sum(zf ** 2, dim=1, keepdim=True) + torch.sum(emb ** 2, dim=1) - 2 * torch.einsum('bd,dn->bn', zf, emb.t())
    zq = emb[torch.argmin(d, dim=1)].view(zp.shape)
    return (zp + (zq - zp)).permute(0, 3, 1, 2).contiguous()


@torch.no_grad()
def ddim_update_opts(x, e_t, a_t, a_prev, sigma_t, sq1m, noise=None, temperature=1.0, keep=None, p=0.0, codebook=None):
    """ddim.py:195-210 with the options: noise = sigma z * temperature, dropout (keep: bool tensor, scaled by 1 / (1 - p)), pred_x0
    quantized to the codebook. noise None: no noise term (sigma * noise == 0)."""
    b = x.shape[0]
    full = lambda v: torch.full((b, 1, 1, 1), v, dtype=torch.float32)
    A, AP, SG, SQ = full(a_t), full(a_prev), full(sigma_t), full(sq1m)
    pred_x0 = (x - SQ * e_t) / A.sqrt()
    if codebook is not None:
        pred_x0 = vq_quantize(pred_x0, codebook)
    dir_xt = (1.0 - AP - SG ** 2).sqrt() * e_t
    nz = SG * (noise if noise is not None else torch.zeros_like(x)) * temperature
    if keep is not None:
        nz = nz * (keep.float().div_(1 - p))
    return AP.sqrt() * pred_x0 + dir_xt + nz, pred_x0


@torch.no_grad()
def ddim_opts_sample(apply_model, sched, x_T, cond, S, eta=0.0, uncond=None, scale=1.0, noises=None, temperature=1.0, keeps=None, p=0.0,
                     codebook=None, rescale_phi=0.7):
    """The reference's loop (ddim.py:113-162, 164-210) with the options; noises[i] / keeps[i]: iteration i's draw and keep mask."""
    ds = oddim.DDIMSchedule(sched, S, eta)
    ts = ds.ddim_timesteps
    total = ts.shape[0]
    img, b = x_T, x_T.shape[0]
    pred = []
    for i, step in enumerate(np.flip(ts)):
        index = total - i - 1
        t = torch.full((b,), int(step), dtype=torch.long)
        if uncond is None or scale == 1.0:
            e_t = apply_model(img, t, cond)
        else:
            e_t = oddim.cfg_combine(apply_model(img, t, cond), apply_model(img, t, uncond), scale, rescale_phi)
        img, x0 = ddim_update_opts(img, e_t, *ds.scalars(index), None if noises is None else noises[i], temperature,
                                   None if keeps is None else keeps[i], p, codebook)
        pred.append(x0)
    return img, pred


def toy_eps(x, t, c):
    """the closed-form eps model of F10 / F17 / F21"""
    tf = t.float()[:, None, None, None] / 1000.0
    return torch.tanh(x * (0.5 + tf) + c["bias"]) * (0.8 + 0.3 * tf) + 0.1 * c["bias"]


def f21_case(fx, case):
    """keyword arguments of ddim_opts_sample for F21 case `case` (CPU tensors; the recorded noises and masks rebuilt from their recipes)"""
    o = F21_CASES[case]
    T = lambda k: torch.from_numpy(np.asarray(fx[k]))
    shape = tuple(fx["xT"].shape)
    kw = dict(x_T=T("xT"), cond={"bias": T("cond")}, S=F21_S, eta=o["eta"], temperature=o.get("temperature", 1.0),
              noises=[prng.normal(F21_SEED, f"opts.{case}.n{k}", shape) for k in range(F21_S)])
    if "cfg" in o:
        kw.update(uncond={"bias": T("uncond")}, scale=o["cfg"])
    if o.get("noise_dropout", 0.0) > 0:
        p = o["noise_dropout"]
        kw.update(p=p, keeps=[prng.uniform(F21_SEED, f"opts.{case}.d{k}", shape, lo=0.0, hi=1.0) >= p for k in range(F21_S)])
    if o.get("quantize_x0"):
        kw["codebook"] = T("codebook")
    return kw


def rel(a, b):
    a, b = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.std())


# ------------------------------------------------------------------------------------------------ F21 and the keep rule
def test_f21_loop_matches_the_reference_sampler(golden):
    fx = golden("f21_ddim_opts")
    sched = oddim.Schedule()
    for case in F21_CASES:
        calls = [0]

        def am(x, t, c):
            calls[0] += 1
            return toy_eps(x, t, c)

        out, pred = ddim_opts_sample(am, sched, **f21_case(fx, case))
        assert calls[0] == int(fx[f"{case}_calls"])
        err = rel(out, fx[f"{case}_out"])
        assert err < 1e-5, (case, err)
        assert rel(torch.stack(pred), fx[f"{case}_pred_x0"]) < 1e-5, case
        if F21_CASES[case].get("quantize_x0"):          # every pred_x0 pixel is a codebook row
            cb = torch.from_numpy(fx["codebook"])
            px = torch.from_numpy(fx[f"{case}_pred_x0"]).permute(0, 1, 3, 4, 2).reshape(-1, cb.shape[1])
            assert float(torch.cdist(px.double(), cb.double()).min(dim=1).values.max()) < 1e-5      # up to the straight-through rounding


def test_f21_options_change_the_result(golden):
    """Each option moves the sample away from the plain loop (the fixture exercises them)."""
    fx = golden("f21_ddim_opts")
    sched = oddim.Schedule()
    for case in F21_CASES:
        kw = f21_case(fx, case)
        plain = {k: v for k, v in kw.items() if k not in ("temperature", "keeps", "p", "codebook")}
        ref, _ = ddim_opts_sample(toy_eps, sched, **plain)
        assert rel(ref, fx[f"{case}_out"]) > 1e-4, case


def test_keep_rule_rate_scale_and_sample_keying():
    n = 3 * 64 * 64
    for p in (0.1, 0.2, 0.5):
        k = keep_mask(77, range(8), n, 3, p)
        rate = float(k.mean())
        sd = np.sqrt(p * (1 - p) / k.size)
        assert abs(rate - (1 - p)) < 5 * sd, (p, rate)
    k0 = keep_mask(77, range(8), n, 3, 0.2)
    assert np.array_equal(keep_mask(77, range(4, 8), n, 3, 0.2), k0[4:])          # keyed by the global sample id, not by position
    assert not np.array_equal(keep_mask(77, range(8), n, 4, 0.2), k0)             # a new mask every iteration
    assert not np.array_equal(keep_mask(78, range(8), n, 3, 0.2), k0)
    assert keep_mask(77, range(2), n, 3, 0.0).all()
    assert drop_scale(0.2) == float(np.float32(1.25)) and drop_scale(0.5) == 2.0


# ------------------------------------------------------------------------------------------------ the sampler's option handling (no GPU)
class _CPUToy:
    """Duck-typed model for DDIMSampler on the CPU: the ops it would call are replaced by recorders in these tests."""
    def __init__(self, codebook=None):
        s = oddim.Schedule()
        self.num_timesteps = 1000
        self.alphas_cumprod = s.alphas_cumprod
        self.device = torch.device("cpu")
        if codebook is not None:
            self.first_stage_model = type("FS", (), {})()
            self.first_stage_model.quantize = type("Q", (), {})()
            self.first_stage_model.quantize.embedding = torch.nn.Embedding(codebook.shape[0], codebook.shape[1])
            self.first_stage_model.quantize.embedding.weight.data.copy_(codebook)

    def apply_model(self, x, t, c):
        return toy_eps(x, t, c)


@pytest.fixture
def recorded(monkeypatch):
    from stedm_amd import ops
    calls = []
    monkeypatch.setattr(ops, "ddim_step", lambda *a, **k: calls.append(("ddim_step", k)))
    monkeypatch.setattr(ops, "ddim_step_ex", lambda *a, **k: calls.append(("ddim_step_ex", k)))
    monkeypatch.setattr(ops, "ddim_quantize_x0", lambda *a, **k: calls.append(("ddim_quantize_x0", dict(k, codebook=a[3]))))
    return calls


def _args():
    return dict(conditioning={"bias": torch.zeros(2, 3, 8, 8)}, verbose=False, x_T=torch.zeros(2, 3, 8, 8))


def test_refusals_raise_before_device_work(recorded):
    from stedm_amd.ddim import DDIMSampler
    smp = DDIMSampler(_CPUToy())
    with pytest.raises(NotImplementedError):
        smp.sample(5, 2, (3, 8, 8), quantize_x0=True, **_args())                 # no VQ first stage
    with pytest.raises(ValueError):
        DDIMSampler(_CPUToy(torch.zeros(16, 4))).sample(5, 2, (3, 8, 8), quantize_x0=True, **_args())    # codebook width 4 != C = 3
    with pytest.raises(ValueError):
        smp.sample(5, 2, (3, 8, 8), eta=1.0, noise_dropout=1.0, **_args())
    with pytest.raises(NotImplementedError):
        smp.sample(5, 2, (3, 8, 8), score_corrector=object(), **_args())
    smp.make_schedule(5, verbose=False)
    x = torch.zeros(2, 3, 8, 8)
    t = torch.full((2,), 1, dtype=torch.long)
    for kw in (dict(use_original_steps=True), dict(repeat_noise=True), dict(score_corrector=object())):
        with pytest.raises(NotImplementedError):
            smp.p_sample_ddim(x, {"bias": x}, t, 0, **kw)
    assert recorded == []


def test_eta0_keeps_the_plain_step(recorded):
    from stedm_amd.ddim import DDIMSampler
    DDIMSampler(_CPUToy()).sample(5, 2, (3, 8, 8), eta=0.0, temperature=0.5, noise_dropout=0.3, noise_seed=5, **_args())
    assert [c[0] for c in recorded] == ["ddim_step"] * 5 and all(c[1]["noise"] is None for c in recorded)


def test_sample_accepts_the_options(recorded):
    """temperature / noise_dropout / quantize_x0 reach the kernels (the sampler used to raise NotImplementedError)."""
    from stedm_amd.ddim import DDIMSampler
    cb = prng.normal(3, "o.cb", (16, 3))
    DDIMSampler(_CPUToy(cb)).sample(5, 2, (3, 8, 8), eta=1.0, temperature=0.7, noise_dropout=0.2, quantize_x0=True, noise_seed=11,
                                    sample_id0=4, **_args())
    names = [c[0] for c in recorded]
    assert names == ["ddim_step_ex", "ddim_quantize_x0"] * 5
    ex = recorded[0][1]
    assert ex["draw"] and ex["noise"] is None and ex["temperature"] == 0.7 and ex["noise_dropout"] == 0.2
    assert ex["seed"] == 11 and ex["first_id"] == 4 and ex["n_iters"] == 5
    assert ex["eps_out"] is not None and ex["noise_out"] is not None
    assert torch.equal(recorded[1][1]["codebook"], cb)
    recorded.clear()
    torch.manual_seed(0)
    DDIMSampler(_CPUToy()).sample(5, 2, (3, 8, 8), eta=0.5, noise_dropout=0.2, **_args())      # no noise_seed: torch's noise, seed per call
    assert [c[0] for c in recorded] == ["ddim_step_ex"] * 5
    assert all(not c[1]["draw"] and c[1]["noise"] is not None for c in recorded)
    assert len({c[1]["seed"] for c in recorded}) == 1
