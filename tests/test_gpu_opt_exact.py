"""GPU tier (-m gpu): the optimizer kernels called by name, no trainer and no U-Net. adamw_ema_kernel, adamw_ema_pack_kernel and
ema_update_kernel (stedm_amd/csrc/opt.hip) through all eleven entry points, on pointer tables built here the way UNetTrainer._build_opt,
_chunks and _fused_opt build them.

What each output is held to (tests/refs_opt.py, pinned on the CPU by tests/test_opt_refs_cpu.py):
  p, m, v, ema     inside the derived per-element bounds of the float64 step, on the designated inputs (gradients over twelve decades, exact
                   zeros, fresh / running / inconsistent state); the largest error-to-bound ratio per output is printed
  ema_update       each word is one of the two fp32 roundings of s - omd (s - p), computed exactly on the CPU
  pack words       equal to refs_pack.words(frag16 / frag32(logical(the kernel's own updated p))), rows beyond cout untouched
  _sched / _clip   the bits of the plain form called with the same scalars (coefficient exactly 1.0), the bound with a coefficient < 1
  everything else  guard words around every buffer, tensors and chunks a launch does not name, the gradients: bits unchanged
Shapes: lengths around the 4096-element chunk and the 4-element vector, two tensors one float off a 16-byte boundary (the scalar path on whole
chunks), a third of the tensors without a shadow, a shuffled chunk list, a chunk list that names part of the table; pack tables with a
one-block descriptor first and in the middle, 1, 2 and 4 outputs, cout != cin, a row count that is no multiple of 128."""
import struct

import numpy as np
import pytest
import torch

from tests import refs_opt as RO
from tests import refs_pack as RP

pytestmark = pytest.mark.gpu

torch.set_grad_enabled(False)

B1, B2, EPS = 0.9, 0.999, 1e-8
G = 64                         # guard words on each side of every buffer (256 B of fp32: the data stays 16-byte aligned)
SENT = 0x7FC0BEEF              # fp32 guard word: a NaN no arithmetic here produces
SENT16 = 0x7FFF                # pack guard word: a NaN in f16 and in bf16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from stedm_amd import ops as o
    return o


class Guarded:
    """data words with G guard words before and after (and `mis` more before: a view that starts mis words past the aligned start)"""

    def __init__(self, data: np.ndarray, dev, mis: int = 0):
        t = torch.from_numpy(np.ascontiguousarray(data))
        self.wdt, self.sent = (torch.int32, SENT) if t.element_size() == 4 else (torch.int16, SENT16)
        self.n, self.lo = t.numel(), G + mis
        self.raw = torch.full((self.lo + self.n + G,), self.sent, dtype=self.wdt, device=dev)
        self.data = self.raw[self.lo:self.lo + self.n]
        self.data.copy_(t.view(self.wdt))
        self.ptr = self.data.data_ptr()
        assert self.ptr % 16 == (mis * t.element_size()) % 16

    def bits(self) -> np.ndarray:
        return self.data.cpu().numpy().copy()

    def guards_ok(self) -> bool:
        r = self.raw.cpu()
        return bool((r[:self.lo] == self.sent).all() and (r[self.lo + self.n:] == self.sent).all())


def _f(bits: np.ndarray) -> np.ndarray:
    return bits.view(np.float32)


def _shuffle(items, tag):
    from stedm_amd.utils import prng
    order = np.argsort(prng.uniform(RO.SEED, f"opt.perm.{tag}", (len(items),), 0.0, 1.0).numpy(), kind="stable")
    return [items[i] for i in order]


def _sched(S, row, dev):
    """a [4][4] device schedule with this step's scalars in `row` and another step's (other lr, other decay) everywhere else"""
    other = RO.sched_row(RO.scalars(S.step + 7, 3.0 * S.lr, S.wd, 0.5))
    rows = [RO.sched_row(S) if i == row else other for i in range(4)]
    return torch.tensor(rows, dtype=torch.float32, device=dev), torch.tensor([row], dtype=torch.int32, device=dev)


def _call(ops, pack, form, c, args, dev, step=None, row=2):
    """one optimizer launch of case c. form: plain | clip | sched | sched_clip (| sched0: the schedule's row 0)"""
    step = c.step if step is None else step
    S = RO.scalars(step, c.lr, c.wd, c.decay, c.grad_scale, c.clip_coef)
    coef = None
    if form.endswith("clip"):
        coef = torch.tensor([1.0 if c.clip_coef is None else c.clip_coef], dtype=torch.float32, device=dev)
    if form.startswith("sched"):
        sched, idx = _sched(S, 0 if form.startswith("sched0") else row, dev)
        fn = ops.adamw_ema_pack_sched if pack else ops.adamw_ema_sched
        fn(*args, B1, B2, EPS, c.wd, sched, idx, grad_scale=c.grad_scale, clip_coef=coef)
    else:
        fn = ops.adamw_ema_pack if pack else ops.adamw_ema
        fn(*args, c.lr, B1, B2, EPS, c.wd, step, c.decay, grad_scale=c.grad_scale, clip_coef=coef)
    torch.cuda.synchronize()


def _inside(host, got, S, worst, what):
    """got[k]: the kernel's bits of output k; host: the fp32 inputs (e None: no shadow). Updates worst[k] and asserts the bound."""
    p, g, m, v, e = host
    ref, bnd = RO.step64(p, g, m, v, e, S), RO.bounds(p, g, m, v, e, S)
    r = RO.ratios({k: _f(got[k]) for k in ref}, ref, bnd)
    for k, x in r.items():
        worst[k] = max(worst.get(k, 0.0), x)
    assert all(x <= 1.0 for x in r.values()), (what, r)
    z = (g == 0) & (m == 0) & (v == 0)          # nothing to accumulate: the moments stay +0 and p moves by the decay alone
    assert not got["m"][z].any() and not got["v"][z].any()
    cw32 = [np.float32(1.0) - np.float32(S.lr) * np.float32(S.wd), RO.fma32(-np.float32(S.lr), np.float32(S.wd), np.float32(1.0))]
    assert all(any(_f(got["p"])[i] == p[i] * cw for cw in cw32) for i in np.flatnonzero(z)), what


def _report(kernel, what, worst):
    print(f"[opt bounds, GPU] {kernel} {what}: largest error / bound  " + "  ".join(f"{k} {worst[k]:.3f}" for k in RO.OUTS if k in worst))


# ------------------------------------------------------------------------------------------------ plain kernel
ALL = dict.fromkeys("pgmve", 1)
# (elements, {stream: words past the 16-byte boundary}, has a shadow, tag of the values). 7 and 9 hold the same values, aligned and not.
TENSORS = [(1, {}, True, "t0"), (3, {}, True, "t1"), (4, {}, False, "t2"), (255, {}, True, "t3"), (4095, {}, False, "t4"), (4096, {}, True, "t5"),
           (4097, {}, False, "t6"), (8192, {}, True, "t7"), (8192 + 5, {}, False, "t8"), (8192, ALL, True, "t7"), (4096 + 7, {"m": 1}, True, "t10")]
ALIGNED, MISALIGNED = 7, 9


class PlainTable:
    def __init__(self, c, dev, with_moments=True):
        self.host, self.bufs, rows = [], [], []
        for n, mis, has_e, tag in TENSORS:
            x = RO.elements(c, tag, n)
            names = "pgmve" if has_e else "pgmv"
            if not with_moments:
                names = "pe" if has_e else "p"
            b = {k: Guarded(x["pgmve".index(k)], dev, mis.get(k, 0)) for k in names}
            self.host.append(x[:4] + (x[4] if has_e else None,))
            self.bufs.append(b)
            rows.append([b[k].ptr if k in b else 0 for k in "pgmve"] + [n])
        self.table = torch.tensor(rows, dtype=torch.int64, device=dev)
        self.chunks = _shuffle([(i, o) for i, t in enumerate(TENSORS) for o in range(0, t[0], 4096)], "plain")
        self.dev = dev

    def lists(self, chunks=None):
        ch = self.chunks if chunks is None else chunks
        return (self.table, torch.tensor([t for t, _ in ch], dtype=torch.int32, device=self.dev),
                torch.tensor([o for _, o in ch], dtype=torch.int64, device=self.dev))

    def snap(self):
        return [{k: b.bits() for k, b in bs.items()} for bs in self.bufs]

    def guards_ok(self):
        return all(b.guards_ok() for bs in self.bufs for b in bs.values())


def _same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(x[k], y[k]), (what, i, k)


def _run_plain(ops, c, dev, form, **kw):
    t = PlainTable(c, dev)
    _call(ops, False, form, c, t.lists(), dev, **kw)
    assert t.guards_ok(), (c.name, form)
    return t, t.snap()


@pytest.mark.parametrize("case", [c.name for c in RO.CASES])
def test_adamw_ema_inside_bounds(dev, ops, case):
    """one launch over the whole table (shuffled chunks): every element of p, m, v and ema inside the bounds, guards and gradients intact;
    the clip cases go through stedm_adamw_ema_clip with the coefficient on the device"""
    c = RO.CASE[case]
    form = "plain" if c.clip_coef is None else "clip"
    t, got = _run_plain(ops, c, dev, form)
    S, worst = RO.case_scalars(c), {}
    for i, (host, o) in enumerate(zip(t.host, got)):
        assert np.array_equal(_f(o["g"]), host[1]), i
        assert ("e" in o) == TENSORS[i][2]
        _inside(host, o, S, worst, (case, i))
    _report("adamw_ema_kernel", f"{case} ({form})", worst)
    diff = [k for k in got[ALIGNED] if not np.array_equal(got[ALIGNED][k], got[MISALIGNED][k])]
    if diff:
        print(f"note: the scalar path (mis-aligned views) and the 16-byte path differ in bits for {diff} on equal inputs; both are inside the bounds")


def test_adamw_ema_subset_chunk_list_leaves_the_rest_alone(dev, ops):
    """what the overlapped optimizer's per-bucket runs launch: a chunk list that names some tensors, and of two tensors only some chunks. The
    named chunks take a second step (inside the bounds from the first step's outputs); every other word keeps its bits."""
    c = RO.CASE["step1000"]
    t, first = _run_plain(ops, c, dev, "plain")
    named = [(8, 8192), (3, 0), (MISALIGNED, 0), (8, 0), (ALIGNED, 4096)]
    _call(ops, False, "plain", c, t.lists(named), dev, step=c.step + 1)
    assert t.guards_ok()
    second = t.snap()
    S, worst = RO.scalars(c.step + 1, c.lr, c.wd, c.decay, c.grad_scale), {}
    for i, (a, b) in enumerate(zip(first, second)):
        n = TENSORS[i][0]
        sel = np.zeros(n, dtype=bool)
        for ti, o in named:
            if ti == i:
                sel[o:o + 4096] = True
        for k in a:
            assert np.array_equal(a[k][~sel], b[k][~sel]), (i, k)
        if sel.any():
            host = tuple(_f(a[k])[sel] if k in a else None for k in "pgmve")
            _inside(host, {k: b[k][sel] for k in b}, S, worst, ("second step", i))
    _report("adamw_ema_kernel", "second step on named chunks", worst)


@pytest.mark.parametrize("case,form,base", [("fresh", "sched0", "plain"), ("step1000", "sched", "plain"), ("clip_one", "clip", "plain"),
                                            ("clip_one", "sched_clip", "plain"), ("clip", "sched_clip", "clip"), ("clip", "sched0_clip", "clip")])
def test_adamw_ema_sched_and_clip_forms_give_the_plain_bits(dev, ops, case, form, base):
    """_sched: row 0 and row 2 of a device schedule {bc1, sqrt(bc2), decay, lr} whose other rows state another step. _clip with a coefficient
    of exactly 1.0 against the entry point without one; with 0.37, the scheduled form against the host-scalar form."""
    c = RO.CASE[case]
    if base == "plain":
        c0 = c._replace(clip_coef=None)
        assert c.clip_coef in (None, 1.0)
    else:
        c0 = c
    _, want = _run_plain(ops, c0, dev, base)
    _, got = _run_plain(ops, c, dev, form)
    _same_bits(want, got, (case, form))


# ------------------------------------------------------------------------------------------------ stedm_ema_update
@pytest.mark.parametrize("case", ["fresh", "step1000"])
def test_ema_update_is_one_of_the_two_roundings(dev, ops, case):
    """LitEma alone over the optimizer's table shapes (g, m, v null, as UNetTrainer._build_ema leaves them): every shadow word equals the
    unfused or the fused fp32 rounding of s - omd (s - p); the parameters, the guards and the tensors without a shadow are untouched"""
    c = RO.CASE[case]
    t = PlainTable(c, dev, with_moments=False)
    before = t.snap()
    ops.ema_update(*t.lists(), c.decay)
    torch.cuda.synchronize()
    assert t.guards_ok()
    after = t.snap()
    S, n_unf, n_fus, n_all = RO.case_scalars(c), 0, 0, 0
    for i, (host, a, b) in enumerate(zip(t.host, before, after)):
        assert np.array_equal(a["p"], b["p"]), i
        if host[4] is None:
            assert "e" not in b
            continue
        unf, fus = RO.ema_candidates(host[4], host[0], S)
        u, f = b["e"] == unf.view(np.int32), b["e"] == fus.view(np.int32)
        assert (u | f).all(), (i, int((~(u | f)).sum()))
        n_unf, n_fus, n_all = n_unf + int(u.sum()), n_fus + int(f.sum()), n_all + u.size
    print(f"[ema_update {case}] {n_all} words: {n_unf} equal the unfused rounding, {n_fus} the fused one")


# ------------------------------------------------------------------------------------------------ fused pack kernel
STRAIGHT16, STRAIGHT32, DGRAD16, DGRAD32 = (0, 1), (0, 0), (1, 1), (1, 0)          # (transposed + flipped, 16x16x32 kind)
# (cout, cin, taps), has a shadow, outputs ((kind), precision). A one-block weight first and in the middle; 1, 2 and 4 outputs.
WEIGHTS = [
    ((32, 32, 1), True, [(STRAIGHT16, "f16")]),
    ((32, 64, 9), True, [(STRAIGHT16, "f16"), (STRAIGHT32, "bf16"), (DGRAD16, "bf16"), (DGRAD32, "f16")]),
    ((32, 32, 1), True, [(DGRAD32, "bf16"), (STRAIGHT32, "f16")]),
    ((96, 32, 9), True, [(STRAIGHT16, "bf16"), (STRAIGHT32, "f16"), (DGRAD16, "f16"), (DGRAD32, "bf16")]),
    ((64, 96, 1), False, [(DGRAD16, "f16"), (STRAIGHT16, "bf16")]),
    ((160, 32, 9), True, [(STRAIGHT16, "f16"), (STRAIGHT32, "bf16"), (DGRAD16, "f16"), (DGRAD32, "bf16")]),
]


def _pack_geometry(shape, kind):
    """-> (rows, channels, sn, sc, flip, fragment order) of one output: the straight strides, or (taps, cin taps, flip) for the dgrad order"""
    (cout, cin, taps), (tr, m16) = shape, kind
    order = RP.frag16 if m16 else RP.frag32
    return ((cin, cout, taps, cin * taps, 1, order) if tr else (cout, cin, cin * taps, taps, 0, order))


class PackTable:
    def __init__(self, c, dev, ops):
        prow, pciw = ops.adamw_ema_pack_piece()
        self.host, self.bufs, self.outs, rec, blk = [], [], [], [], 0
        for wi, (shape, has_e, outs) in enumerate(WEIGHTS):
            cout, cin, taps = shape
            assert cout % prow == 0 and cin % pciw == 0, f"{shape} is not whole pieces of {prow} x {pciw}: choose other shapes"
            x = RO.elements_long(c, f"w{wi}", cout * cin * taps)
            names = "pgmve" if has_e else "pgmv"
            b = {k: Guarded(x["pgmve".index(k)], dev) for k in names}
            self.host.append(x[:4] + (x[4] if has_e else None,))
            self.bufs.append(b)
            body, ob = b"", []
            for kind, prec in outs:
                R, Cc, _, _, _, order = _pack_geometry(shape, kind)
                valid = order(torch.ones(R, Cc, taps)) != 0           # the words of rows < R; the others belong to nobody
                o = Guarded(np.full(valid.numel(), SENT16, dtype=np.int16), dev)
                ob.append((o, valid))
                body += struct.pack("<Qiiii", o.ptr, kind[0], kind[0], kind[1], int(prec == "f16"))
            self.outs.append(ob)
            rec.append(struct.pack("<QQQQQiiiiii", *[b[k].ptr if k in b else 0 for k in "pgmve"], cout, cin, taps, blk, len(outs), 0) +
                       body + b"\0" * (24 * (4 - len(outs))))
            assert len(rec[-1]) == 160
            blk += (cout // prow) * (cin // pciw)
        self.n, self.blocks = len(rec), blk
        self.descs = torch.frombuffer(bytearray(b"".join(rec)), dtype=torch.uint8).to(dev)

    def args(self):
        return (self.descs, self.n, self.blocks)

    def snap(self):
        return [{k: b.bits() for k, b in bs.items()} for bs in self.bufs]

    def packs(self):
        return [[o.bits() for o, _ in ob] for ob in self.outs]

    def guards_ok(self):
        return all(b.guards_ok() for bs in self.bufs for b in bs.values()) and all(o.guards_ok() for ob in self.outs for o, _ in ob)


def _run_pack(ops, c, dev, form):
    t = PackTable(c, dev, ops)
    assert t.n >= 4 and {len(w[2]) for w in WEIGHTS} == {1, 2, 4}
    _call(ops, True, form, c, t.args(), dev)
    assert t.guards_ok(), (c.name, form)
    return t, t.snap(), t.packs()


def _plain_on_pack_inputs(ops, c, dev, form):
    """the plain kernel over the same weights as flat tensors (aligned, whole chunk list in order)"""
    bufs, rows = [], []
    for wi, (shape, has_e, _) in enumerate(WEIGHTS):
        x = RO.elements_long(c, f"w{wi}", shape[0] * shape[1] * shape[2])
        b = {k: Guarded(x["pgmve".index(k)], dev) for k in ("pgmve" if has_e else "pgmv")}
        bufs.append(b)
        rows.append([b[k].ptr if k in b else 0 for k in "pgmve"] + [x[0].size])
    ch = [(i, o) for i, r in enumerate(rows) for o in range(0, r[5], 4096)]
    args = (torch.tensor(rows, dtype=torch.int64, device=dev), torch.tensor([t for t, _ in ch], dtype=torch.int32, device=dev),
            torch.tensor([o for _, o in ch], dtype=torch.int64, device=dev))
    _call(ops, False, form, c, args, dev)
    return [{k: b.bits() for k, b in bs.items()} for bs in bufs]


@pytest.mark.parametrize("case", ["fresh", "step1000", "tiny_v", "clip"])
def test_adamw_ema_pack_against_the_references(dev, ops, case):
    """p, m, v, ema: the plain kernel's bits and inside the bounds. Every pack word of a row < cout (dgrad order: < cin) equals the reference
    rounding of the kernel's own updated p in the reference layout; the other words and the guards keep the sentinel."""
    c = RO.CASE[case]
    form = "plain" if c.clip_coef is None else "clip"
    t, got, packs = _run_pack(ops, c, dev, form)
    _same_bits(_plain_on_pack_inputs(ops, c, dev, form), got, (case, "plain kernel"))
    S, worst = RO.case_scalars(c), {}
    for wi, (host, o) in enumerate(zip(t.host, got)):
        assert np.array_equal(_f(o["g"]), host[1]), wi
        _inside(host, o, S, worst, (case, wi))
        shape, _, outs = WEIGHTS[wi]
        pnew = torch.from_numpy(_f(o["p"]).copy())
        for oi, ((kind, prec), (_, valid), words) in enumerate(zip(outs, t.outs[wi], packs[wi])):
            R, Cc, sn, sc, flip, order = _pack_geometry(shape, kind)
            want = RP.words(order(RP.logical(pnew, sn, sc, flip, R, Cc, shape[2])), prec)
            want = torch.where(valid, want, torch.full_like(want, SENT16)).reshape(-1)
            assert valid.any() and (R % 128 == 0 or not valid.all())
            assert torch.equal(torch.from_numpy(words), want), (case, wi, oi, kind, prec, int((torch.from_numpy(words) != want).sum()))
    _report("adamw_ema_pack_kernel", f"{case} ({form})", worst)


@pytest.mark.parametrize("case,form,base", [("fresh", "sched0", "plain"), ("step1000", "sched", "plain"), ("clip_one", "clip", "plain"),
                                            ("clip", "sched_clip", "clip")])
def test_adamw_ema_pack_sched_and_clip_forms_give_the_plain_bits(dev, ops, case, form, base):
    c = RO.CASE[case]
    c0 = c._replace(clip_coef=None) if base == "plain" else c
    assert base != "plain" or c.clip_coef in (None, 1.0)
    _, want, wpacks = _run_pack(ops, c0, dev, base)
    _, got, gpacks = _run_pack(ops, c, dev, form)
    _same_bits(want, got, (case, form))
    for wi, (a, b) in enumerate(zip(wpacks, gpacks)):
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), (case, form, wi)
