"""Plain torch restatements of the two conv-less resampling kernels (stedm_amd/csrc/resample.hip; include/stedm_hip.h), NHWC, with the
producer-side channel statistics for ANY partition of a sample's output pixels into slots. Pinned against F.avg_pool2d / F.interpolate in
tests/test_resample_refs_cpu.py; the GPU tests (tests/test_gpu_resample_kernels.py) hold the kernels against them bit for bit on dyadic
inputs, where every sum and square is exact in fp32 whatever the order of additions."""
import torch


def avgpool2x2(x: torch.Tensor) -> torch.Tensor:
    """[B][H][W][C] -> [B][H/2][W/2][C], 0.25 * (((a00 + a01) + a10) + a11) in x's dtype: the kernel's order of additions"""
    assert x.shape[1] % 2 == 0 and x.shape[2] % 2 == 0, "avgpool2x2: H and W must be even"
    return 0.25 * (((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + x[:, 1::2, 0::2]) + x[:, 1::2, 1::2])


def replicate2x2(x: torch.Tensor, scale: float = 1.0, prior: torch.Tensor = None) -> torch.Tensor:
    """[B][H][W][C] -> [B][2H][2W][C]: out[b][2y+dy][2x+dx][c] = (prior +) scale * x[b][y][x][c], the product rounded first"""
    v = (x * torch.tensor(scale, dtype=x.dtype)).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    return v if prior is None else prior + v


def pool_slots(Ho: int, Wo: int) -> torch.Tensor:
    """slot of every output pixel of stedm_avgpool2x2 [Ho][Wo]: runs of 256 output pixels"""
    return (torch.arange(Ho * Wo) // 256).view(Ho, Wo)


def replicate_slots(H: int, W: int) -> torch.Tensor:
    """slot of every output pixel of stedm_replicate2x2 [2H][2W] for an input [H][W]: the four copies of a run of 64 input pixels"""
    return (torch.arange(H * W) // 64).view(H, W).repeat_interleave(2, dim=0).repeat_interleave(2, dim=1)


def nslab(Ho: int, Wo: int) -> int:
    """slot count of both kernels for an output of Ho x Wo pixels: stedm_gn_chan_nslab(Ho * Wo)"""
    return (Ho * Wo + 255) // 256


def chan_stats(out: torch.Tensor, slots: torch.Tensor, n: int = None) -> torch.Tensor:
    """chan_stats [B][n][C][2] = {sum, sum of squares} of out [B][Ho][Wo][C] over the pixels of each slot (slots [Ho][Wo], integer), in fp64"""
    B, Ho, Wo, C = out.shape
    n = int(slots.max()) + 1 if n is None else n
    o = out.double().reshape(B, Ho * Wo, C)
    cs = torch.zeros((B, n, C, 2), dtype=torch.float64)
    idx = slots.reshape(-1).long()
    cs[..., 0].index_add_(1, idx, o)
    cs[..., 1].index_add_(1, idx, o * o)
    return cs


def fold(cs: torch.Tensor) -> torch.Tensor:
    """what every consumer does with the slots: adds them -> [B][C][2]"""
    return cs.sum(dim=1)


def dyadic(gen: torch.Generator, shape) -> torch.Tensor:
    """multiples of 1/8 with magnitude <= 2: sums of four, their quarter, squares and sums of thousands of those are exact in fp32"""
    return torch.randint(-16, 17, tuple(shape), generator=gen).float() / 8
