"""GPU tier (-m gpu): masked DDIM sampling (DDIMSampler.sample's mask / x0, reference ddim.py:143-146) on the HIP sampler.
  * the blend kernel (stedm_ddim_mask_blend) against an fp32 torch restatement, every mask broadcast, a row length off the float4 grid;
    its in-kernel noise draw bit for bit against stedm_philox_normal, and shard-invariant;
  * the sampler against F17 (the reference's own masked sampler, recorded noises) and, with the TINY U-Net, against the masked oracle
    loop of tests/test_masked_sampler_oracle.py, eager and hipGraph replay;
  * graph == eager and mask == 0 == unmasked, bit for bit;
  * predict_latents / predict_latents_sharded with an image-resolution mask and a real VQ-f4 first stage."""
import numpy as np
import pytest
import torch

from stedm_amd.utils import prng
from tests.test_masked_sampler_oracle import f17_case, masked_ddim_sample, toy_eps

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
MASK_STREAM = 0x8000


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.std())


def _tables(dev):
    from oracle import ddim as od
    s = od.Schedule()
    return s.sqrt_alphas_cumprod.to(dev), s.sqrt_one_minus_alphas_cumprod.to(dev)


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("B,C,h,w", [(3, 4, 8, 8), (3, 3, 5, 7)])        # (5 x 7: planes and rows off the float4 grid, row length 105)
def test_blend_kernel_matches_torch_for_every_mask_broadcast(dev, B, C, h, w):
    from stedm_amd import ops
    sa, s1 = _tables(dev)
    x0 = prng.normal(40, "k.x0", (B, C, h, w)).to(dev)
    img = prng.normal(40, "k.img", (B, C, h, w)).to(dev)
    noise = prng.normal(40, "k.noise", (B, C, h, w)).to(dev)
    t = torch.tensor([1, 501, 981][:B], dtype=torch.int64, device=dev)
    for mb, mc in ((B, 1), (1, 1), (B, C), (1, C)):
        for soft in (False, True):
            u = prng.uniform(40, f"k.mask{mb}{mc}", (mb, mc, h, w), lo=0.0, hi=1.0)
            mask = (u if soft else (u > 0.5).float()).to(dev)
            want = (sa[t].view(B, 1, 1, 1) * x0 + s1[t].view(B, 1, 1, 1) * noise) * mask + (1.0 - mask) * img
            got = ops.ddim_mask_blend(img.clone(), x0, mask, t, sa, s1, noise=noise)
            err = float((got - want).abs().max())
            assert err <= 1e-6, (mb, mc, soft, err)
            keep = mask.expand(B, C, h, w) == 0
            assert torch.equal(got[keep], img[keep])          # 0 * q + 1 * img is img exactly
    with pytest.raises(ValueError):
        ops.ddim_mask_blend(img.clone(), x0, torch.ones(2, 2, h, w, device=dev), t, sa, s1, noise=noise)
    with pytest.raises(ValueError):
        ops.ddim_mask_blend(img.clone(), x0[:1].contiguous(), torch.ones(1, 1, h, w, device=dev), t, sa, s1, noise=noise)


@pytest.mark.parametrize("B,C,h,w", [(5, 4, 16, 16), (5, 3, 5, 7)])
def test_in_kernel_noise_is_philox_normal_bit_for_bit_and_shard_invariant(dev, B, C, h, w):
    from stedm_amd import ops
    sa, s1 = _tables(dev)
    x0 = prng.normal(41, "n.x0", (B, C, h, w)).to(dev)
    img = prng.normal(41, "n.img", (B, C, h, w)).to(dev)
    mask = prng.uniform(41, "n.mask", (B, 1, h, w), lo=0.0, hi=1.0).to(dev)
    t = torch.full((B,), 301, dtype=torch.int64, device=dev)
    seed, first_id = 0x1234ABCD5678, 7
    for index in (0, 3):
        step = torch.tensor([index], dtype=torch.int32, device=dev)
        drawn = ops.ddim_mask_blend(img.clone(), x0, mask, t, sa, s1, step_idx=step, seed=seed, first_id=first_id)
        nz = ops.philox_normal(B, (C, h, w), seed, MASK_STREAM + index, dev, first_id=first_id)
        given = ops.ddim_mask_blend(img.clone(), x0, mask, t, sa, s1, noise=nz, seed=seed, first_id=first_id)
        assert torch.equal(drawn, given), index
        shard = ops.ddim_mask_blend(img[2:].clone(), x0[2:].contiguous(), mask[2:].contiguous(), t[2:], sa, s1, step_idx=step, seed=seed,
                                    first_id=first_id + 2)
        assert torch.equal(shard, drawn[2:]), index
    assert not torch.equal(drawn, ops.ddim_mask_blend(img.clone(), x0, mask, t, sa, s1, step_idx=torch.zeros(1, dtype=torch.int32, device=dev),
                                                      seed=seed, first_id=first_id))


# ------------------------------------------------------------------------------------------------ F17 through the HIP sampler
class GpuToy:
    """The closed-form eps model of F17 on the device, with the model surface the sampler reads (schedule buffers, device)."""

    def __init__(self, dev):
        from oracle import ddim as od
        s = od.Schedule()
        self.num_timesteps = 1000
        self.betas = s.betas.to(dev)
        self.alphas_cumprod = s.alphas_cumprod.to(dev)
        self.sqrt_alphas_cumprod = s.sqrt_alphas_cumprod.to(dev)
        self.sqrt_one_minus_alphas_cumprod = s.sqrt_one_minus_alphas_cumprod.to(dev)
        self.device = dev
        self.calls = 0

    def apply_model(self, x, t, c, **kw):
        self.calls += 1
        return toy_eps(x, t, c)


def test_f17_on_the_hip_sampler(dev, golden):
    from stedm_amd.ddim import DDIMSampler
    fx = golden("f17_ddim_mask")
    for case in ("a", "b"):
        kw = f17_case(fx, case)
        toy = GpuToy(dev)
        d = lambda c: None if c is None else {"bias": c["bias"].to(dev)}
        extra = {} if case == "b" else dict(unconditional_conditioning=d(kw["uncond"]), unconditional_guidance_scale=1.5, log_every_t=5)
        if case == "b":
            extra["noises"] = kw["noises"]
        s, inter = DDIMSampler(toy).sample(kw["S"], 2, (4, 8, 8), d(kw["cond"]), verbose=False, eta=kw["eta"], x_T=kw["x_T"].to(dev),
                                           mask=kw["mask"].to(dev), x0=kw["x0"].to(dev), mask_noises=kw["q_noises"], **extra)
        assert toy.calls == int(fx[f"{case}_calls"])
        err = rel(s, fx[f"{case}_out"])
        print(f"[F17 {case} on the HIP sampler] max|diff|/std {err:.3e}")
        assert err < 1e-4, case
        if case == "a":
            assert len(inter["x_inter"]) == 6
            assert rel(torch.stack(inter["x_inter"]), fx["a_x_inter"]) < 1e-4


def test_mask_argument_rules(dev):
    from stedm_amd.ddim import DDIMSampler
    toy = GpuToy(dev)
    xT = torch.zeros(2, 4, 8, 8, device=dev)
    c = {"bias": torch.zeros(2, 4, 8, 8, device=dev)}
    m = torch.ones(2, 1, 8, 8, device=dev)
    smp = DDIMSampler(toy)
    with pytest.raises(ValueError):                                    # mask without x0 (the reference asserts)
        smp.sample(2, 2, (4, 8, 8), c, verbose=False, x_T=xT, mask=m)
    with pytest.raises(ValueError):                                    # a batch-1 x0 is not broadcast
        smp.sample(2, 2, (4, 8, 8), c, verbose=False, x_T=xT, mask=m, x0=torch.zeros(1, 4, 8, 8, device=dev))
    with pytest.raises(ValueError):
        smp.sample(2, 2, (4, 8, 8), c, verbose=False, x_T=xT, mask=torch.ones(2, 2, 8, 8, device=dev), x0=xT)
    with pytest.raises(NotImplementedError):
        smp.sample(2, 2, (4, 8, 8), c, verbose=False, x_T=xT, mask=m, x0=xT, quantize_x0=True)


# ------------------------------------------------------------------------------------------------ TINY U-Net loop
def _tiny_inputs(B=2):
    from tests.test_gpu_sampler import inputs
    xT, cc, ctx, ctx_u = inputs(B)
    x0 = prng.normal(42, "m.x0", (B, 4, 16, 16))
    mask = torch.zeros(B, 1, 16, 16)
    mask[..., :8] = 1.0                                                 # keep the left half
    return xT, cc, ctx, ctx_u, x0, mask


def _tiny_sample(dev, use_graph, precision, mask, x0, mask_seed=None, S=5):
    from tests.test_gpu_sampler import make
    xT, cc, ctx, ctx_u, _, _ = _tiny_inputs()
    ld = make(dev, use_graph, precision)
    cond = {"c_concat": [cc.to(dev)], "c_crossattn": [ctx.to(dev)]}
    unc = {"c_concat": [cc.to(dev)], "c_crossattn": [ctx_u.to(dev)]}
    kw = {} if mask is None else dict(mask=mask.to(dev), x0=x0.to(dev), mask_seed=mask_seed)
    s, inter = ld.sample_log(cond, 2, True, S, eta=0.0, x_T=xT.to(dev), unconditional_conditioning=unc, unconditional_guidance_scale=1.5,
                             log_every_t=1000, **kw)
    return s.clone(), inter


def test_tiny_unet_masked_loop_vs_oracle_eager_and_graph(dev):
    from oracle import ddim as od
    from oracle import dropmask as odm
    from oracle import unet as ou
    xT, cc, ctx, ctx_u, x0, mask = _tiny_inputs()
    seed, S, B = 2024, 5, 2
    total = od.make_ddim_timesteps(S).shape[0]
    q_noises = [torch.from_numpy(odm.normal_rows(seed, range(B), 4 * 16 * 16, MASK_STREAM + total - 1 - i)).view(B, 4, 16, 16)
                for i in range(total)]
    cfg = ou.UNetConfig(image_size=16, in_channels=7, model_channels=32, out_channels=4, channel_mult=(1, 2, 4), num_heads=4)
    plan = ou.build_plan(cfg)
    P = prng.fill_state_dict(plan.shapes, 6)
    am = lambda x, t, c: ou.unet_forward(P, cfg, torch.cat([x, c["c_concat"][0]], 1), t, c["c_crossattn"][0], plan=plan)
    ref, _ = masked_ddim_sample(am, od.Schedule(), xT, {"c_concat": [cc], "c_crossattn": [ctx]}, S, mask, x0, q_noises,
                                uncond={"c_concat": [cc], "c_crossattn": [ctx_u]}, scale=1.5)
    for use_graph in (False, True):
        s, _ = _tiny_sample(dev, use_graph, "parity", mask, x0, mask_seed=seed, S=S)
        err = rel(s, ref)
        print(f"[masked ddim cfg x5, graph={use_graph}] rel err vs the masked oracle loop: {err:.3e}")
        assert err < 1e-3


def test_masked_graph_equals_eager_bits(dev):
    _, _, _, _, x0, mask = _tiny_inputs()
    outs = [_tiny_sample(dev, g, "f16", mask, x0, mask_seed=99)[0] for g in (False, True)]
    assert torch.equal(outs[0], outs[1])
    other = _tiny_sample(dev, True, "f16", mask, x0, mask_seed=100)[0]
    assert not torch.equal(other, outs[1])                              # the seed reaches the replayed draw


def test_all_zero_mask_is_the_unmasked_sample_bit_for_bit(dev):
    _, _, _, _, x0, mask = _tiny_inputs()
    for g in (False, True):
        plain, pi = _tiny_sample(dev, g, "f16", None, None)
        zero, zi = _tiny_sample(dev, g, "f16", torch.zeros_like(mask), x0, mask_seed=5)
        assert torch.equal(plain, zero), g
        assert len(pi["x_inter"]) == len(zi["x_inter"]) and all(torch.equal(a, b) for a, b in zip(pi["x_inter"], zi["x_inter"]))


# ------------------------------------------------------------------------------------------------ prediction entry points
B_PRED, STEPS_PRED, SEED_PRED = 4, 4, 61


def _pred_model(dev):
    """S_ZSS_DM with a tiny VQ-f4 first stage (64^2 images -> 16^2 latents: get_input really encodes), a small U-Net on 16^2 latents,
    the sViT style encoder and the SpatialRescaler; parity mode, hipGraph replay."""
    from stedm_amd.latent_diffusion import S_ZSS_DM
    from stedm_amd.unet import UNetModel
    from tests.test_gpu_vq import DD_TINY
    ucfg = dict(image_size=16, in_channels=7, model_channels=128, out_channels=4, num_res_blocks=1,
                attention_resolutions=[32, 16, 8], channel_mult=[1, 2], num_heads=4)
    unet = UNetModel(**ucfg).eval()
    prng.fill_module_(unet, seed=50)
    agg = dict(name="svit", patch_size=8, dim=256, depth=2, heads=12, mlp_dim=256, pool="mean", channels=3, dropout=0.1, emb_dropout=0.1, t_dim=256)
    first = {"target": "stedm_amd.vq.VQModelInterface",
             "params": dict(embed_dim=4, n_embed=256, ddconfig=dict(DD_TINY, z_channels=4), lossconfig={"target": "torch.nn.Identity"})}
    model = S_ZSS_DM("swin_v2_t", dict(name="mp", num_patches=4), agg, {"data": {"patch_size": 64}}, unet, linear_start=0.0015, linear_end=0.0205,
                     image_size=16, channels=4, conditioning_key="hybrid", loss_type="l1", cond_stage_key="segmentation", use_graph=True,
                     first_stage_config=first, cond_stage_config={"target": "ldm.modules.encoders.modules.SpatialRescaler",
                                                                  "params": {"n_stages": 2, "in_channels": 2, "out_channels": 3}})
    prng.fill_module_(model.agg_block, seed=51)
    prng.fill_module_(model.cond_stage_model, seed=52)
    prng.fill_module_(model.first_stage_model, seed=19)
    return model.to(dev).eval()


def _pred_batch(ids, dev):
    from stedm_amd import parallel as par
    img = par.per_sample_normal(SEED_PRED, ids, (64, 64, 3), stream=300).clamp(-1, 1)
    seg = (par.per_sample_normal(SEED_PRED, ids, (64, 64, 2), stream=301) > 0).float()
    sty = par.per_sample_normal(SEED_PRED, ids, (4, 64, 64, 3), stream=302).clamp(-1, 1)
    return {"image": img.to(dev), "segmentation": seg.to(dev), "style_imgs": sty.to(dev)}


def test_predict_latents_with_an_image_mask(dev):
    from stedm_amd.latent_diffusion import predict_latents, predict_latents_sharded
    from stedm_amd import parallel as par
    model = _pred_model(dev)
    ids = list(range(B_PRED))
    batch = _pred_batch(ids, dev)
    # image mask: keep the left half, with a few single-pixel holes that must drop their whole 4 x 4 latent footprint
    im = torch.zeros(B_PRED, 64, 64)
    im[:, :, :32] = 1.0
    im[0, 5, 9] = 0.0
    im[1, 40, 30] = 0.0
    im[2, 17, 2] = 0.5
    want = np.ones((B_PRED, 1, 16, 16), dtype=np.float32)
    for b in range(B_PRED):
        for y in range(16):
            for x in range(16):
                want[b, 0, y, x] = float(im[b, 4 * y:4 * y + 4, 4 * x:4 * x + 4].min())
    lat_mask = torch.from_numpy(want)
    assert float(lat_mask.sum()) == B_PRED * 16 * 8 - 2 - 0.5
    z = model.get_input(batch, "image", predict_only=False)[0]
    assert float(z.abs().max()) > 0
    xT = prng.normal(SEED_PRED, "p.xT", (B_PRED, 4, 16, 16)).to(dev)
    run = lambda **kw: predict_latents(model, batch, STEPS_PRED, cfg_scale=1.5, style_sampling="mp", x_T=xT, mask_seed=7, **kw)
    a = run(mask=im.to(dev))                                            # x0 from the batch's own image, image mask min-pooled
    b = run(mask=lat_mask.to(dev), x0=z)
    assert torch.equal(a, b)
    assert not torch.equal(a, run(mask=lat_mask.to(dev), x0=torch.zeros_like(z)))
    kept = (lat_mask.to(dev) == 1).expand_as(a)
    assert float((a - z)[kept].abs().mean()) < float((a - z)[~kept].abs().mean())
    # two half-shards on one device against the world-1 run (x_T and the blend's noise keyed by the global sample id)
    full = predict_latents_sharded(model, batch, B_PRED, STEPS_PRED, cfg_scale=1.5, seed=SEED_PRED, rank=0, world=1, gather=False,
                                   style_sampling="mp", mask=im.to(dev))
    parts = []
    for r in range(2):
        lo, hi = par.shard_range(B_PRED, r, 2)
        parts.append(predict_latents_sharded(model, _pred_batch(list(range(lo, hi)), dev), B_PRED, STEPS_PRED, cfg_scale=1.5, seed=SEED_PRED,
                                             rank=r, world=2, gather=False, style_sampling="mp", mask=im.to(dev)))
    got = torch.cat(parts).double().cpu()
    ref = full.double().cpu()
    per = ((got - ref).flatten(1).abs().amax(1) / ref.flatten(1).std(1)).tolist()
    print(f"[masked predict, 2 x 2 vs 1 x 4, parity] worst sample max|diff|/std {max(per):.3e}")
    assert max(per) < 1e-3
