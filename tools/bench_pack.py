"""A/B timing of the weight packs across library builds: python tools/bench_pack.py libA.so libB.so ... [--rounds N]

Every library is loaded into this one process and the rounds alternate between them in a rotating order (a round = 20 back-to-back launches
of one case on one library between two device events), so clock and neighbour drift hits all builds alike. Reported per case and library: the median and
the minimum over the rounds, in microseconds per launch. Naming one library twice gives the noise floor of the comparison."""
import ctypes as C, os, statistics, struct, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stedm_amd.ops import pack_blocks

dev = torch.device("cuda:0")
BF16, INNER = 1, 20
ceil128 = lambda n: (n + 127) // 128


def cases():
    """(name, bytes moved, call(lib)): outputs are allocated once and shared by the libraries"""
    out = []
    i16 = lambda *shape: torch.empty(shape, dtype=torch.int16, device=dev)
    for co, ci, ks in [(1024, 1024, 3), (512, 1536, 3), (128, 128, 3), (3072, 1024, 1)]:
        w, taps = torch.randn(co, ci, ks, ks, device=dev), ks * ks
        f32, f16, hl = i16(ceil128(co), ci // 16, taps, 4, 64, 8), i16(ceil128(co), ci // 32, taps, 8, 64, 8), i16(2, ceil128(co), ci // 32, taps, 8, 64, 8)
        tag = f"{co}x{ci}x{ks}x{ks}"
        out.append((f"frag   fwd {tag}", w.numel() * 6, lambda L, w=w, o=f32, a=(co, ci, ks): L.stedm_pack_conv_weight_frag(w.data_ptr(), o.data_ptr(), *a, BF16, None)))
        out.append((f"frag16 fwd {tag}", w.numel() * 6, lambda L, w=w, o=f16, a=(co, ci, ks), s=(ci * taps, taps): L.stedm_pack_conv_weight_frag16(
            w.data_ptr(), *s, 0, o.data_ptr(), *a, BF16, None)))
        hl_fn = "stedm_pack_conv_weight_frag16_hl" if ks == 3 else "stedm_pack_conv_weight_frag16_hl1"
        out.append((f"frag16 hi+lo {tag}", w.numel() * 8, lambda L, w=w, o=hl, a=(co, ci), s=(ci * taps, taps), fn=hl_fn: getattr(L, fn)(
            w.data_ptr(), *s, 0, o.data_ptr(), *a, BF16, None)))
        if ks == 3:      # the dgrad filter: rows = forward input channels, taps reversed, straight from the OIHW parameter
            d32, d16 = i16(ceil128(ci), co // 16, taps, 4, 64, 8), i16(ceil128(ci), co // 32, taps, 8, 64, 8)
            out.append((f"frag   dgrad {tag}", w.numel() * 6, lambda L, w=w, o=d32, a=(ci, co, ks), s=(taps, ci * taps): L.stedm_pack_conv_weight_strided(
                w.data_ptr(), *s, 1, None, None, o.data_ptr(), *a, BF16, None)))
            out.append((f"frag16 dgrad {tag}", w.numel() * 6, lambda L, w=w, o=d16, a=(ci, co, ks), s=(taps, ci * taps): L.stedm_pack_conv_weight_frag16(
                w.data_ptr(), *s, 1, o.data_ptr(), *a, BF16, None)))
    dy, o3 = torch.randn(4096, 1024, device=dev), i16(8, 4096 // 16, 1, 4, 64, 8)
    out.append(("frag   dyT 4096x1024", dy.numel() * 6, lambda L: L.stedm_pack_conv_weight_strided(dy.data_ptr(), 1, 1024, 0, None, None, o3.data_ptr(), 1024, 4096, 1, BF16, None)))
    for co, ci in [(1024, 1024), (512, 512)]:      # Upsample / Downsample convolutions
        w = torch.randn(co, ci, 3, 3, device=dev)
        up, up16 = i16(4, ceil128(co), ci // 16, 4, 4, 64, 8), i16(2, 4, ceil128(co), ci // 32, 4, 8, 64, 8)
        sd, sd16 = i16(ceil128(co), 4 * ci // 16, 4, 4, 64, 8), i16(2, ceil128(co), 4 * ci // 32, 4, 8, 64, 8)
        pl = i16(2, 4 * co, 4, ci)
        tag = f"{co}x{ci}"
        out.append((f"up planes hi+lo {tag}", w.numel() * 4 + pl.numel() * 2, lambda L, w=w, o=pl, a=(co, ci): L.stedm_pack_conv_weight_up(w.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), *a, BF16, None)))
        out.append((f"up_frag {tag}", w.numel() * 4 + up.numel() * 2, lambda L, w=w, o=up, a=(co, ci): L.stedm_pack_conv_weight_up_frag(w.data_ptr(), o.data_ptr(), *a, BF16, None)))
        out.append((f"up_frag16 hi+lo {tag}", w.numel() * 4 + up16.numel() * 2, lambda L, w=w, o=up16, a=(co, ci): L.stedm_pack_conv_weight_up_frag16_hl(w.data_ptr(), o.data_ptr(), *a, BF16, None)))
        out.append((f"s2d_frag {tag}", w.numel() * 4 + sd.numel() * 2, lambda L, w=w, o=sd, a=(co, ci): L.stedm_pack_conv_weight_s2d_frag(w.data_ptr(), o.data_ptr(), *a, BF16, 0, None)))
        out.append((f"s2d_frag16 hi+lo {tag}", w.numel() * 4 + sd16.numel() * 2, lambda L, w=w, o=sd16, a=(co, ci): L.stedm_pack_conv_weight_s2d_frag16_hl(w.data_ptr(), o.data_ptr(), *a, BF16, 0, None)))
    # one stedm_pack_frag_multi table of training-step size: every 3x3 / 1x1 convolution of a 128-channel, (1, 4, 8)-multiplier U-Net, each in
    # the forward order and in the transposed + flipped dgrad order (16x16x32 from 256 contracted channels on, 32x32x16 below)
    shapes = [(128, 128, 3)] * 4 + [(512, 128, 3), (512, 512, 3), (512, 128, 1)] + [(512, 512, 3)] * 6 + [(1024, 512, 3), (1024, 1024, 3), (1024, 512, 1)] + \
             [(1024, 1024, 3)] * 10 + [(1024, 2048, 3), (1024, 2048, 1)] * 3 + [(1024, 1536, 3), (1024, 1536, 1), (512, 1536, 3), (512, 1536, 1)] + \
             [(512, 1024, 3), (512, 1024, 1)] * 2 + [(512, 640, 3), (512, 640, 1), (128, 640, 3), (128, 640, 1)] + [(128, 256, 3), (128, 256, 1)] * 2
    rec, keep, blk, nbytes = [], [], 0, 0
    for co, ci, ks in shapes:
        w, taps = torch.randn(co, ci, ks, ks, device=dev), ks * ks
        for (n, c, sn, sc, flip) in ((co, ci, ci * taps, taps, 0), (ci, co, taps, ci * taps, 1)):
            m16 = int(ks == 3 and c >= 256)
            o = i16(ceil128(n), c // (32 if m16 else 16), taps, 8 if m16 else 4, 64, 8)
            rec.append(struct.pack("<QQqqiiiiii", w.data_ptr(), o.data_ptr(), sn, sc, n, c, taps, flip, m16, blk))
            blk += pack_blocks(n, c, m16)
            keep += [w, o]
            nbytes += w.numel() * 4 + o.numel() * 2
    table = torch.frombuffer(bytearray(b"".join(rec)), dtype=torch.uint8).to(dev)
    out.append((f"pack_frag_multi {len(rec)} tensors", nbytes, lambda L, k=keep: L.stedm_pack_frag_multi(table.data_ptr(), len(rec), blk, BF16, None)))
    return out


def load(path):
    L = C.CDLL(path)
    P, I, Lg = C.c_void_p, C.c_int, C.c_long
    for name, args in {"stedm_pack_conv_weight_frag": [P, P, I, I, I, I, P], "stedm_pack_conv_weight_strided": [P, Lg, Lg, I, P, P, P, I, I, I, I, P],
                       "stedm_pack_conv_weight_frag16": [P, Lg, Lg, I, P, I, I, I, I, P], "stedm_pack_conv_weight_frag16_hl": [P, Lg, Lg, I, P, I, I, I, P],
                       "stedm_pack_conv_weight_frag16_hl1": [P, Lg, Lg, I, P, I, I, I, P], "stedm_pack_conv_weight_up": [P, P, P, I, I, I, P],
                       "stedm_pack_conv_weight_up_frag": [P, P, I, I, I, P], "stedm_pack_conv_weight_up_frag16_hl": [P, P, I, I, I, P],
                       "stedm_pack_conv_weight_s2d_frag": [P, P, I, I, I, I, P], "stedm_pack_conv_weight_s2d_frag16_hl": [P, P, I, I, I, I, P],
                       "stedm_pack_frag_multi": [P, I, I, I, P]}.items():
        getattr(L, name).argtypes, getattr(L, name).restype = args, I
    return L


def main():
    argv = sys.argv[1:]
    rounds = int(argv.pop(argv.index("--rounds") + 1)) if "--rounds" in argv else 15
    paths = [a for a in argv if a != "--rounds"]
    libs = [load(p) for p in paths]
    for i, p in enumerate(paths):
        print(f"[{i}] {p}")
    print(f"{'case':34s}" + "".join(f"  [{i}] median    min" for i in range(len(libs))) + "   (us per launch; GB/s at the first library's median)")
    for name, nbytes, call in cases():
        for L in libs:
            for _ in range(3):
                assert call(L) == 0, name
        torch.cuda.synchronize()
        ts = [[] for _ in libs]
        for r in range(rounds):
            for i in [(r + j) % len(libs) for j in range(len(libs))]:      # the order rotates: no build always follows the same one
                L = libs[i]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(INNER):
                    call(L)
                e1.record()
                torch.cuda.synchronize()
                ts[i].append(e0.elapsed_time(e1) / INNER * 1e3)
        med = [statistics.median(t) for t in ts]
        print(f"{name:34s}" + "".join(f"  {m:10.2f} {min(t):6.2f}" for m, t in zip(med, ts)) + f"   {nbytes / med[0] / 1e3:7.1f}", flush=True)


if __name__ == "__main__":
    main()
