"""In-tree counterpart of the reference's Lightning wrapper `modules/ldm_diffusion.py::LDM_Diffusion` (:14-234) for the HIP path.

Same constructor argument (the Hydra config), same members the drivers call — `prepare_batch` (:51-60), `training_step(batch,
batch_idx)` (:63-73), `predict_step` (:76-107), `on_train_batch_start/end` (:110-115), `on_train_epoch_end` (:118-221; its eight
monitoring images come from two batched DDIM runs, `sample_test_images`), `configure_optimizers` (:224-234) — with one
declared difference: `automatic_optimization = False`. The training step runs the fused HIP path (`S_ZSS_DM.training_step_hip`:
forward + L1 + hand-scheduled backward, gradient accumulation, bucketed all-reduce over the ranks, fused AdamW + EMA), so Lightning's
own backward / DDP reducer / optimizer loop have nothing to do; `train_diff.py` can construct this class in place of the reference's
and call `Trainer.fit` with `strategy=DDPStrategy(...)` for the process group alone. Where pytorch_lightning is not installed (this
repository's test boxes) the class derives from `torch.nn.Module` and is driven by a plain loop that makes the same calls in the same
order (tests/test_gpu_train.py::test_ldm_module_training_loop_as_the_reference_drives_it).

A maintainer who wants to keep Lightning's automatic optimisation and torch.optim.AdamW instead uses `S_ZSS_DM.training_step` (the
reference's own seam, autograd bridge in latent_diffusion.py) and `attach_optimizer` for the cross-rank average.
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .latent_diffusion import S_ZSS_DM, images_for_saving, predict_latents, prepare_batch

try:  # pragma: no cover - not installed on the test boxes
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except ImportError:
    pl = None
    _Base = nn.Module


class _Cfg(dict):
    """attribute access over a plain nested dict (the reference passes an OmegaConf DictConfig; both work)"""

    def __getattr__(self, k):
        try:
            v = self[k]
        except KeyError as e:
            raise AttributeError(k) from e
        return _Cfg(v) if isinstance(v, dict) and not isinstance(v, _Cfg) else v


def _to_container(c):
    if isinstance(c, dict):
        return {k: _to_container(v) for k, v in c.items()}
    try:  # OmegaConf, when present
        from omegaconf import OmegaConf
        return OmegaConf.to_container(c)
    except ImportError:
        return c


class LDM_Diffusion(_Base):
    def __init__(self, cfg, wandb_id: str = "", accumulate_grad_batches: int = 4):
        super().__init__()
        cfg = _Cfg(cfg) if isinstance(cfg, dict) and not isinstance(cfg, _Cfg) else cfg
        self._cfg = cfg
        self._lr = cfg.lr
        self._wandb_id = wandb_id
        self.automatic_optimization = False
        # Trainer(accumulate_grad_batches=4) is hard-coded in train_diff.py:76; with manual optimisation the module owns the window
        self._accumulate = int(accumulate_grad_batches)
        ldm_dict = dict(_to_container(cfg.diffusion))
        fs = ldm_dict.get("first_stage_config")
        if isinstance(fs, dict) and isinstance(fs.get("params"), dict) and fs["params"].get("ckpt_path") and hasattr(cfg, "location"):
            fs["params"]["ckpt_path"] = cfg.location.result_dir + "/" + fs["params"]["ckpt_path"]      # ldm_diffusion.py:30
        ldm_dict.pop("ckpt_path", None)
        # optional config key (default false: the reference as wired): train the set-ViT style encoder with the U-Net
        tse = getattr(cfg, "train_style_encoder", False)
        self._model = S_ZSS_DM(encoder="swin_v2_t", sampling_cfg=cfg.style_sampling, agg_cfg=cfg.style_agg, cfg=cfg,
                               train_style_encoder=bool(tse), **ldm_dict)
        self.register_module("model", self._model)          # state-dict aliasing of ldm_diffusion.py:38-41: `_model.*` and `model.*`
        self._loss_sum, self._loss_n = None, 0          # device-side accumulator (the reference's MeanMetric, ldm_diffusion.py:44)
        self.predict_dir: Optional[str] = None

    def forward(self, x, *args, **kwargs):
        return self._model.forward(x, *args, **kwargs)

    def prepare_batch(self, batch):
        """ldm_diffusion.py:51-60."""
        return prepare_batch(batch, device=self._model.device)

    # ------------------------------------------------------------------------------------------ training
    def configure_optimizers(self):
        """ldm_diffusion.py:224-234: AdamW(lr) over model.model (+ cond_stage_model while cond_stage_trainable; the aggregation block is
        not in the reference's list). Built as the fused HIP optimizer; Lightning gets no optimizer object (manual optimisation) — and
        refuses `Trainer(gradient_clip_val=...)` for that reason, so the optional config keys `gradient_clip_val` / `gradient_clip_algorithm`
        (Lightning's names) are read here instead; configs without them run as before. A `scheduler_config` under cfg.diffusion reaches
        the trainer through the model (LatentDiffusion.configure_trainer)."""
        cfg = self._cfg
        self._model.configure_trainer(lr=self._lr, accumulate_grad_batches=self._accumulate, gradient_clip_val=getattr(cfg, "gradient_clip_val", None),
                                      gradient_clip_algorithm=getattr(cfg, "gradient_clip_algorithm", None) or "norm")
        return None

    def training_step(self, batch, batch_idx):
        """ldm_diffusion.py:63-73 with the fused step in place of `loss = self._model.training_step(ldm_batch, batch_idx)` + Lightning's
        backward / optimizer loop."""
        ldm_batch = self.prepare_batch(batch)
        m = self._model
        if m.__dict__.get("_trainer") is None:
            self.configure_optimizers()
        x, c = m.get_input(ldm_batch, m.first_stage_key)[:2]
        loss = m.training_step_hip(x, c)
        # MeanMetric of ldm_diffusion.py:44,71: accumulated on the device — no host sync per micro-batch; train_loss() converts once
        ld = loss.detach().float().reshape(())
        self._loss_sum = ld.clone() if self._loss_sum is None else self._loss_sum + ld
        self._loss_n += 1
        return loss

    def on_train_batch_start(self, batch, batch_idx):
        """ldm_diffusion.py:110-112 -> ddpm.py:479-494, which returns at once unless scale_by_std is set and this is batch 0: the batch is
        only prepared (a seg_merge kernel plus copies) when that rescale will actually run."""
        m = self._model
        if not (getattr(m, "scale_by_std", False) and batch_idx == 0):
            return
        m.on_train_batch_start(self.prepare_batch(batch), batch_idx, -1)

    def on_train_batch_end(self, *args, **kwargs):
        self._model.on_train_batch_end(*args, **kwargs)

    def train_loss(self, reset: bool = True) -> float:
        """what on_train_epoch_end logs as "Train Loss" (ldm_diffusion.py:118-120)"""
        v = 0.0 if self._loss_sum is None else float(self._loss_sum) / max(1, self._loss_n)
        if reset:
            self._loss_sum, self._loss_n = None, 0
        return v

    # ------------------------------------------------------------------------------------------ epoch end
    @torch.no_grad()
    def sample_test_images(self, test_folder: Optional[str] = None, ddim_steps: int = 128, seed: Optional[int] = None):
        """The monitoring images of ldm_diffusion.py:127-221 -> {"Sample Images": [4 uint8 [H,W,3] arrays], "Sample Images CFG": [4 arrays]
        (absent when no guided run is made)}.

        Files read as the reference reads them, from `test_folder` (default cfg.location.data_dir + "/" + cfg.data.test_folder):
        test_c.png (grey, > 0 -> class 1, one-hot over 2 classes) and, under the style sampling's name, the four test styles:
        "nearby" {i}_img.png; "mp" {i}_img_{k}.png for k < num_patches; "dummy" no files, the constant stack zeros / 127.5 - 1 (at the
        condition image's size; the reference hard-codes 512). Pixels / 127.5 - 1, first three channels.

        The reference renders each image in a run of its own: eight batch-1 DDIM-128 runs. Here they are two graphed runs at eta 0
        through predict_latents (conditionings from get_input(..., predict_only=True): the reference's VQ encodes of a zero image are
        unused; the unconditional style is encoded once):
          * B = 4 unguided, test styles 0 - 3;
          * B = 4 guided, rows [style 0, style 0, style 1, style 1] at guidance scales [3, 5, 3, 5] against the shared unconditional
            conditioning, one scale per sample (stedm_ddim_step_rows) - only when style_drop_rate > 0 and the sampling is not "dummy"
            (:193).
        Each batch is decoded once and converted by images_for_saving's uint8 rule.

        Declared differences: the reference draws eight independent torch.randn x_T; here x_T are the per-sample Philox streams of
        (seed, sample ids 0 - 3 unguided, 4 - 7 guided), seed defaulting to one draw from torch's CPU generator. The module's train / eval
        flags are restored afterwards (the reference leaves eval() set)."""
        from PIL import Image
        from . import parallel as par
        cfg, m = self._cfg, self._model
        if test_folder is None:
            test_folder = cfg.location.data_dir + "/" + cfg.data.test_folder
        scfg = cfg.style_sampling
        sname = scfg["name"] if isinstance(scfg, dict) else scfg.name
        dev = m.device
        test_img = (np.array(Image.open(os.path.join(test_folder, "test_c.png")).convert("L")) > 0).astype(np.uint8)
        seg = torch.nn.functional.one_hot(torch.from_numpy(test_img).to(torch.long), num_classes=2).unsqueeze(0).to(torch.float32)
        H, W = test_img.shape
        sdir = os.path.join(test_folder, sname)
        load = lambda name: torch.from_numpy(np.array(Image.open(os.path.join(sdir, name)))[:, :, :3]).to(torch.float32)[None, None] / 127.5 - 1
        if sname == "nearby":
            styles = [load(f"{i}_img.png") for i in range(4)]
        elif sname == "mp":
            num = scfg["num_patches"] if isinstance(scfg, dict) else scfg.num_patches
            styles = [torch.cat([load(f"{i}_img_{k}.png") for k in range(num)], dim=1) for i in range(4)]
        elif sname == "dummy":
            styles = [torch.zeros((1, 1, H, W, 3), dtype=torch.float32) / 127.5 - 1] * 4
        else:
            raise ValueError(f"sample_test_images: no test styles are defined for style_sampling {sname!r} (nearby, mp, dummy)")
        guided = float(getattr(cfg, "style_drop_rate", 0.0)) > 0.0 and sname != "dummy"
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())

        def batch_of(rows):
            return {"image": torch.zeros((len(rows), H, W, 3), dtype=torch.float32, device=dev),
                    "segmentation": seg.expand(len(rows), -1, -1, -1).contiguous().to(dev),
                    "style_imgs": torch.cat([styles[i] for i in rows], dim=0).to(dev)}

        shape = (m.channels, m.image_size, m.image_size)
        x_T = (lambda first: par.per_sample_normal_device(seed, first, 4, shape, 0, dev)) if torch.device(dev).type == "cuda" else \
              (lambda first: par.per_sample_normal(seed, list(range(first, first + 4)), shape, stream=0).to(dev))
        flags = [(mod, mod.training) for mod in self.modules()]
        graph = m.use_graph
        out = {}
        try:
            m.eval()
            m.use_graph = True
            runs = [("Sample Images", [0, 1, 2, 3], 1.0, 0)]
            if guided:
                runs.append(("Sample Images CFG", [0, 0, 1, 1], [3.0, 5.0, 3.0, 5.0], 4))
            for title, rows, scale, first in runs:
                lat = predict_latents(m, batch_of(rows), ddim_steps=ddim_steps, eta=0.0, cfg_scale=scale, style_sampling=sname, x_T=x_T(first))
                img, _ = images_for_saving(m.decode_first_stage(lat))
                out[title] = list(img.cpu().numpy())
        finally:
            m.use_graph = graph
            for mod, was in flags:
                mod.training = was
        return out

    def on_train_epoch_end(self):
        """ldm_diffusion.py:118-221: logs "Train Loss" (when the base class offers `log`: under Lightning), records the wandb id (when a
        logger exists), renders the monitoring images when cfg.data has `test_folder` (sample_test_images) and hands them to
        logger.log_image with the reference's titles and captions. The images stay in `last_test_images` ({} without test_folder), so a
        plain loop without Lightning or a logger gets them too."""
        loss = self.train_loss()
        if callable(getattr(self, "log", None)):
            self.log("Train Loss", loss)
        try:
            logger = getattr(self, "logger", None)
        except RuntimeError:          # a LightningModule that no Trainer holds
            logger = None
        if logger is not None and self._wandb_id == "":
            self._wandb_id = logger.version
            if hasattr(self, "hparams"):
                self.hparams["wandb_id"] = self._wandb_id
        self.last_test_images = {}
        data = getattr(self._cfg, "data", None)
        if data is not None and (("test_folder" in data) if isinstance(data, dict) else hasattr(data, "test_folder")):
            self.last_test_images = self.sample_test_images()
            if logger is not None:
                captions = ["Test 0", "Test 1", "Test 2", "Test 3"]
                for title in ("Sample Images CFG", "Sample Images"):          # the reference's order (:213, :221)
                    if title in self.last_test_images:
                        logger.log_image(title, images=self.last_test_images[title], caption=captions)

    # ------------------------------------------------------------------------------------------ prediction
    @torch.no_grad()
    def predict_step(self, batch, batch_idx):
        """ldm_diffusion.py:76-107: conditional + unconditional conditioning, DDIM + CFG, VQ decode, uint8 images and class maps;
        PNG files when `predict_dir` is set. Returns (images [B,H,W,3] uint8, segmentation [B,H,W] uint8) on the host.

        The config key `sampler` (optional; "ddim" when absent, as in the reference's configs) selects "dpm_solver" (DPM-Solver++(2M),
        stedm_amd/dpm_solver.py); `ddim_steps` is then the number of model evaluations (DDIM's uniform stride makes 128 into 143). "plms"
        selects PLMS (stedm_amd/plms.py), DDIM's schedule with n + 1 model evaluations for n iterations. "ddpm" runs the reference's
        ancestral chain (stedm_amd/ancestral.py: model.num_timesteps unguided steps, ddim_steps ignored; cfg_scale must then be 1).
        The optional mapping `dpm_solver` (with sampler "dpm_solver") holds DPM-Solver options (latent_diffusion.DPM_OPTIONS, e.g.
        {order: 3} or {method: singlestep, order: 3}); configs without it run exactly as before. The optional mapping `first_stage_split`
        (the reference's `split_input_params` keys: ks, stride, vqf, patch_distributed_vq, clip_*_weight, tie_braker, clip_*_tie_weight; ks
        and stride in latent pixels) decodes the latents over overlapping crops (LatentDiffusion.decode_first_stage(split=...))."""
        cfg = self._cfg
        ldm_batch = self.prepare_batch(batch)
        sname = cfg.style_sampling["name"] if isinstance(cfg.style_sampling, dict) else cfg.style_sampling.name
        dpm = getattr(cfg, "dpm_solver", None)
        extra = {} if dpm is None else {"dpm_solver": dict(dpm.items() if hasattr(dpm, "items") else vars(dpm).items())}
        scale = cfg.cfg_scale           # a number, or a list-valued key: one guidance scale per sample of the batch (predict_latents)
        if not isinstance(scale, (int, float, torch.Tensor, np.ndarray)) and hasattr(scale, "__len__"):
            scale = [float(v) for v in scale]
        lat = predict_latents(self._model, ldm_batch, ddim_steps=cfg.ddim_steps, eta=cfg.eta, cfg_scale=scale, style_sampling=sname,
                              sampler=getattr(cfg, "sampler", None) or "ddim", **extra)
        split = getattr(cfg, "first_stage_split", None)
        if split is None:
            dec = self._model.decode_first_stage(lat)
            img, seg = images_for_saving(dec, ldm_batch["segmentation"])
        else:       # patch-distributed decode: the uint8 image comes straight out of the blend
            img = self._model.decode_first_stage(lat, split=dict(split.items() if hasattr(split, "items") else vars(split).items()), out_u8=True)
            _, seg = images_for_saving(None, ldm_batch["segmentation"])
        img, seg = img.cpu().numpy(), seg.cpu().numpy()
        if self.predict_dir is not None and len(batch) > 4:
            from PIL import Image
            for im, sg, num in zip(img, seg, batch[4].cpu().numpy()):
                num_str = str(int(num)).zfill(5)
                Image.fromarray(im).save(os.path.join(self.predict_dir, f"img_{num_str}.png"))
                Image.fromarray(sg).save(os.path.join(self.predict_dir, f"seg_{num_str}.png"))
        return img, seg
