"""The GRU step kernels one at a time, against float64, inside guard bands.

csrc/gru_step.hip holds three forward kernels (gru_step_fwd_kernel<0|1|2>, the pipelined gru_step_fwd_a2w3_kernel, the persistent
gru_l1_fwd_persistent_kernel) and one backward kernel with two roles (A: cell + recurrent product, over three operand routes: none /
packed rows / the trie's sum_idx indirection; B: the previous step's input gradient); csrc/rowops.hip holds the unfused cells.  Every
case here launches ONE of them through its C entry point with all outputs carved from NaN-filled allocations (tests_support.Guarded:
bands compared bitwise), all row operands with NaN in their leading-dimension gap and around their rows, and holds every output to
the float64 restatement of tests_support.gru_fwd_bounds / gru_bwd_bounds: first-order error propagation from c_acc, C_OUT and c_fast,
no free tolerance.  For bf16 outputs that is about one ulp of the stored value.

Which case reaches which kernel follows from the dispatch of gtos_gru_step_fwd: mode 2 with hs == 256, no h_idx, no y and
rows >= 16384 -> persistent; mode 1 with rows >= 8192, in_dim % 64 == 0, (in_dim + hs) / 64 % 6 == 0 and no h_idx -> pipelined;
everything else -> gru_step_fwd_kernel<mode>.

The CPU self-checks at the top emulate the kernels in fp32 torch on bf16 operands, rounding where the kernels round: the honest
emulation passes every bound and each of nine plausible kernel mistakes is rejected -- they prove that the GPU assertions can fail."""
import pytest
import torch

from tests_support import (C_OUT, Guarded, assert_bound, assert_within, bias_sum_bound, c_acc, drop_scale, gru_bwd_bounds,
                           gru_fwd_bounds, guarded_operand, within_ratio)

gpu = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
SENT = 3.0                                     # what every output view holds before the launch (exact in bf16)


def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    return torch.device("cuda:0")


def rnd(shape, dtype, device, seed, scale=1.0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + offset).to(dtype).to(device)


def distinct_gather(n_src, n, seed, device):
    """n distinct rows of n_src in a non-identity order (int32)"""
    p = torch.randperm(n_src, generator=torch.Generator().manual_seed(seed))
    if n_src > 1 and bool((p[:n] == torch.arange(n)).all()):
        p = p.roll(1)
    return p[:n].to(torch.int32).to(device)


def hash_keep(seed, idx, p, device):
    from test_hip_parity import _hash_keep
    return _hash_keep(seed, idx.numpy(), p).to(device)


def unchanged(t):
    return bool((t == SENT).all())


# ------------------------------------------------------------------------------------------------ operands and references, forward
def fwd_operands(device, mode, rows, hs, in_dim, h_idx, seed, guard):
    """The stored operands of one forward step; with ``guard`` the row operands sit in NaN (gap of the leading dimension, rows around)."""
    def g(t, **kw):
        return guarded_operand(t, **kw) if guard else t
    o = dict(x=None, w_ih=None, b_ih=None, xg=None, gf=None, gf_idx=None, gb=None, gb_idx=None, h_idx=None)
    n_h = rows + 17 if h_idx else rows
    o["h_in"] = g(rnd((n_h, hs), BF, device, seed + 1))
    if h_idx:
        o["h_idx"] = distinct_gather(n_h, rows, seed + 2, device)
    o["w_hh"] = rnd((3 * hs, hs), BF, device, seed + 3, 0.1)
    o["b_hh"] = rnd((3 * hs,), F32, device, seed + 4, 0.1)
    if mode != 0:
        o["b_ih"] = rnd((3 * hs,), F32, device, seed + 5, 0.1)
    if mode == 1:
        o["x"] = g(rnd((rows, in_dim), BF, device, seed + 6, 0.5), ld=in_dim + 24)
        o["w_ih"] = rnd((3 * hs, in_dim), BF, device, seed + 7, 0.1)
    elif mode == 2:
        nf, nb = 301, 411
        o["gf"] = g(rnd((nf, 3 * hs), BF, device, seed + 6, 0.5))
        o["gb"] = g(rnd((nb, 3 * hs), BF, device, seed + 7, 0.5))
        gen = torch.Generator().manual_seed(seed + 8)
        o["gf_idx"] = torch.randint(0, nf, (rows,), generator=gen).to(torch.int32).to(device)
        o["gb_idx"] = torch.randint(0, nb, (rows,), generator=gen).to(torch.int32).to(device)
    else:
        o["xg"] = g(rnd((rows, 3 * hs), BF, device, seed + 6, 0.7))
    return o


def fwd_refs(mode, o, hn_stored, keep=None, p=0.0):
    """{name: (float64 reference, bound)} of one fused forward step from its stored operands and the kernel's own stored hn."""
    if mode == 1:
        x, w, b = o["x"].double(), o["w_ih"].double(), o["b_ih"].double()
        xg, Sx, k_in = x @ w.t() + b, x.abs() @ w.abs().t() + b.abs(), x.shape[1]
    elif mode == 2:
        f, bk, b = o["gf"].double()[o["gf_idx"].long()], o["gb"].double()[o["gb_idx"].long()], o["b_ih"].double()
        xg, Sx, k_in = f + bk + b, f.abs() + bk.abs() + b.abs(), 0
    else:
        xg = o["xg"].double()
        Sx, k_in = xg.abs(), 0
    h = o["h_in"].double()
    if o["h_idx"] is not None:
        h = h[o["h_idx"].long()]
    w, b = o["w_hh"].double(), o["b_hh"].double()
    hg, Sh = h @ w.t() + b, h.abs() @ w.abs().t() + b.abs()
    return gru_fwd_bounds(xg, Sx, hg, Sh, h, hn_stored, k_in + h.shape[1], BF, keep, p)


def emulate_fwd(o, mutate=None):
    """gru_step_fwd_kernel<1> in fp32 torch on the bf16 operands, rounding hn and the outputs where the kernel does; ``mutate``: one
    deliberate mistake."""
    x, wi, bi = o["x"].float(), o["w_ih"].float(), o["b_ih"].float()
    h, wh, bh = o["h_in"].float(), o["w_hh"].float(), o["b_hh"].float()
    hs = h.shape[1]
    xg, hg = x @ wi.t(), h @ wh.t()
    if mutate == "k stage dropped":                           # the second 64-wide stage of the input product, gate z
        xg[:, hs:2 * hs] -= x[:, 64:128] @ wi[hs:2 * hs, 64:128].t()
    r = torch.sigmoid(xg[:, :hs] + hg[:, :hs] + (bh[:hs] + bi[:hs]))
    z = torch.sigmoid(xg[:, hs:2 * hs] + hg[:, hs:2 * hs] + (bh[hs:2 * hs] + bi[hs:2 * hs]))
    hn, xn = hg[:, 2 * hs:] + bh[2 * hs:], xg[:, 2 * hs:] + bi[2 * hs:]
    if mutate == "b_ih_n into hn":
        hn, xn = hn + bi[2 * hs:], xg[:, 2 * hs:]
    hn_r = hn.to(BF).float()
    n = torch.tanh(xn + r * (hn if mutate == "n from unrounded hn" else hn_r))
    zz = z.to(BF).float() if mutate == "h from rounded z" else z
    out = (1 - zz) * n + zz * h
    return {k: v.to(BF) for k, v in dict(r=r, z=z, n=n, hn=hn_r, h=out, y=out).items()}


FWD_MUTATIONS = ["k stage dropped", "b_ih_n into hn", "n from unrounded hn", "h from rounded z"]


def _cpu_fwd_case():
    return fwd_operands("cpu", 1, 300, 64, 128, False, 100, guard=False)


def test_forward_bounds_accept_the_honest_emulation():
    o = _cpu_fwd_case()
    got = emulate_fwd(o)
    for name, (ref, bound) in fwd_refs(1, o, got["hn"]).items():
        assert_within("emulated forward " + name, got[name], ref, bound)


@pytest.mark.parametrize("mutate", FWD_MUTATIONS)
def test_forward_bounds_reject(mutate):
    o = _cpu_fwd_case()
    got = emulate_fwd(o, mutate)
    ratios = {name: within_ratio(got[name], ref, bound)[0] for name, (ref, bound) in fwd_refs(1, o, got["hn"]).items()}
    print("MUTATION %s: err/bound %s" % (mutate, {k: "%.3g" % v for k, v in ratios.items()}))
    assert max(ratios.values()) > 1.0, ratios


# ------------------------------------------------------------------------------------------------ operands and references, backward
def bwd_operands(device, rows, rows_prev, hs, seed, guard, hprev_idx=False, trie=False, dh_dtype=F32, dy=False):
    def g(t, **kw):
        return guarded_operand(t, **kw) if guard else t
    gen = torch.Generator().manual_seed(seed)
    o = dict(rows=rows, rows_prev=rows_prev, hs=hs, d4_prev=None, wh_t=None, hprev_idx=None, dy=None, sum_idx=None, dh_src=None,
             zero_row=-1)
    n_ = max(rows, 1)
    gates = torch.cat([torch.rand(n_, 2 * hs, generator=gen), torch.rand(n_, hs, generator=gen) * 2 - 1,
                       torch.randn(n_, hs, generator=gen)], 1)
    o["gates"] = g(gates.to(BF).to(device))
    n_hp = n_ + 19 if hprev_idx else n_
    o["hprev"] = g(rnd((n_hp, hs), BF, device, seed + 1))
    if hprev_idx:
        o["hprev_idx"] = distinct_gather(n_hp, n_, seed + 2, device)
    o["dh0"] = rnd((n_, hs), dh_dtype, device, seed + 3)
    if trie:
        n_src = rows // 2 + 5
        o["d4_prev"] = g(rnd((n_src, 4 * hs), BF, device, seed + 4, 0.3))
        o["dh_src"] = g(rnd((n_src, hs), dh_dtype, device, seed + 5))
        s = torch.randint(0, n_src, (rows,), generator=gen)
        s[torch.rand(rows, generator=gen) < 1 / 3] = n_src                 # "all zero": the row right behind both tables (NaN there)
        o["sum_idx"], o["zero_row"] = s.to(torch.int32).to(device), n_src
    elif rows_prev is not None:
        o["d4_prev"] = g(rnd((rows_prev, 4 * hs), BF, device, seed + 4, 0.3))
    if o["d4_prev"] is not None:
        o["wh_t"] = rnd((hs, 3 * hs), BF, device, seed + 6, 0.1)
    if dy:
        o["dy"] = g(rnd((n_, hs), BF, device, seed + 7), ld=2 * hs)
    return o


def bwd_refs(o, keep=None, p=0.0, d4_dtype=BF, dh_dtype=F32):
    """({name: (float64 reference, bound)}, the entering state rows) of role A from the stored operands."""
    rows, hs = o["rows"], o["hs"]
    device = o["gates"].device
    A = torch.zeros(rows, 3 * hs, dtype=torch.float64, device=device)
    dh_in = o["dh0"].double()
    if o["sum_idx"] is not None:
        src = o["sum_idx"].long()
        live = (src != o["zero_row"]).double()[:, None]
        srcc = src.clamp(max=o["d4_prev"].shape[0] - 1)
        d = o["d4_prev"].double()[srcc]
        A = torch.cat([d[:, :2 * hs], d[:, 3 * hs:]], 1) * live
        dh_in = o["dh_src"].double()[srcc] * live
    elif o["d4_prev"] is not None:
        nrec = min(rows, o["rows_prev"])
        d = o["d4_prev"].double()[:nrec]
        A[:nrec] = torch.cat([d[:, :2 * hs], d[:, 3 * hs:]], 1)
    if o["wh_t"] is not None:
        w = o["wh_t"].double()
        P, S_P = A @ w.t(), A.abs() @ w.abs().t()
    else:
        P = S_P = torch.zeros(rows, hs, dtype=torch.float64, device=device)
    dyt = torch.zeros_like(dh_in)
    if o["dy"] is not None:
        dyt = o["dy"].double() * drop_scale(p) * (1.0 if keep is None else keep.double())
    hp = o["hprev"] if o["hprev_idx"] is None else o["hprev"][o["hprev_idx"].long()]
    K = 3 * hs if o["wh_t"] is not None else 1
    return gru_bwd_bounds(o["gates"], hp, dh_in + dyt, dh_in.abs() + dyt.abs(), P, S_P, K, d4_dtype, dh_dtype), hp


def split_d4(d4, hs):
    return dict(dr=d4[:, :hs], dz=d4[:, hs:2 * hs], dn=d4[:, 2 * hs:3 * hs], dhn=d4[:, 3 * hs:])


def emulate_bwd(o, bias0, mutate=None):
    """Role A of gru_step_bwd_kernel (packed route, bf16 dh) in fp32 torch; returns (outputs, bias partials after the launch)."""
    rows, rows_prev, hs = o["rows"], o["rows_prev"], o["hs"]
    gr, gz, gn, hn = (o["gates"][:, i * hs:(i + 1) * hs].float() for i in range(4))
    hp, d4p, w = o["hprev"].float(), o["d4_prev"].float(), o["wh_t"].float()
    A = torch.cat([d4p[:, :2 * hs], d4p[:, 2 * hs:3 * hs] if mutate == "recurrent product reads d n_x" else d4p[:, 3 * hs:]], 1)
    nrec = min(rows, rows_prev)
    P = torch.zeros(rows, hs)
    P[:nrec] = A[:nrec] @ w.t()
    if mutate == "tail row gets a recurrent term":
        P[nrec:] = A[rows_prev - 1] @ w.t()
    g = o["dh0"].float() + P
    dn = g * (1 - gz)
    dz = g * ((gn - hp) if mutate == "dz with (gn - hp)" else (hp - gn))
    dn_ = dn * (1 - gn * gn)
    dhn = dn_ if mutate == "dhn without gr" else dn_ * gr
    dr = dn_ * hn * gr * (1 - gr)
    d4 = torch.cat([dr, dz * gz * (1 - gz), dn_, dhn], 1).to(BF)
    got = dict(split_d4(d4, hs), dh=(g * gz).to(BF))
    sums = d4.float().sum(0)
    if mutate == "last row twice in the bias sums":
        sums = sums + d4[-1].float()
    bias = bias0.clone()
    bias[1] += sums
    return got, d4, bias


BWD_MUTATIONS = ["recurrent product reads d n_x", "dz with (gn - hp)", "dhn without gr", "last row twice in the bias sums",
                 "tail row gets a recurrent term"]


def _bwd_ratios(o, bias0, mutate):
    got, d4, bias = emulate_bwd(o, bias0, mutate)
    refs, _ = bwd_refs(o, dh_dtype=BF)
    ratios = {name: within_ratio(got[name], ref, bound)[0] for name, (ref, bound) in refs.items()}
    ref, bound = bias_sum_bound(d4, o["rows"])
    ratios["bias"] = within_ratio(bias.double().sum(0) - bias0.double().sum(0), ref, bound)[0]
    return ratios


def _cpu_bwd_case():
    return bwd_operands("cpu", 300, 200, 64, 200, guard=False, dh_dtype=BF), rnd((3, 4 * 64), F32, "cpu", 201, 0.05)


def test_backward_bounds_accept_the_honest_emulation():
    o, bias0 = _cpu_bwd_case()
    ratios = _bwd_ratios(o, bias0, None)
    print("MEASURED emulated backward: err/bound %s" % {k: "%.3g" % v for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("mutate", BWD_MUTATIONS)
def test_backward_bounds_reject(mutate):
    o, bias0 = _cpu_bwd_case()
    ratios = _bwd_ratios(o, bias0, mutate)
    print("MUTATION %s: err/bound %s" % (mutate, {k: "%.3g" % v for k, v in ratios.items()}))
    assert max(ratios.values()) > 1.0, ratios


# ------------------------------------------------------------------------------------------------ GPU: the fused forward step
def run_fwd(tag, mode, rows, hs, in_dim=0, n_out=0, fin_idx=False, h_idx=False, y=None, seed=0):
    """One gtos_gru_step_fwd launch, every output guarded, against float64."""
    from gtos_amd._lib import call, ptr, stream
    d = dev()
    o = fwd_operands(d, mode, rows, hs, in_dim, h_idx, seed, guard=True)
    gates = Guarded(rows, 4 * hs, BF, d, init=SENT)
    h_out = Guarded(rows, hs, BF, d, init=SENT)                       # rows n_out.. belong to nobody: they keep SENT
    n_fin, ld_fin = (rows + 13 if fin_idx else rows), 2 * hs + 8
    h_fin = Guarded(n_fin, hs, BF, d, ld=ld_fin, init=SENT)           # a column block of a wider matrix
    fidx = distinct_gather(n_fin, rows, seed + 11, d) if fin_idx else None
    ldy, p, sd, base = 2 * hs, (0.3 if y == "drop" else 0.0), 4242 + seed, 7 * 2 * hs + 24
    yb = Guarded(rows, hs, BF, d, ld=ldy, init=SENT) if y else None
    x = o["x"]
    call("gtos_gru_step_fwd", rows, hs, ptr(x), 0 if x is None else x.stride(0), in_dim, ptr(o["w_ih"]), ptr(o["b_ih"]), ptr(o["xg"]),
         ptr(o["gf"]), ptr(o["gf_idx"]), ptr(o["gb"]), ptr(o["gb_idx"]), ptr(o["h_in"]), ptr(o["h_idx"]), ptr(o["w_hh"]), ptr(o["b_hh"]),
         ptr(h_out.view), n_out, ptr(h_fin.view), ld_fin, ptr(fidx), ptr(gates.view), None if yb is None else ptr(yb.view), ldy,
         p, sd if p > 0 else 0, base, stream())
    for g_, w in ((gates, "gates"), (h_out, "h_out"), (h_fin, "h_fin")) + (((yb, "y"),) if yb else ()):
        g_.check(tag + " " + w)
    keep = None
    if p > 0:
        keep = hash_keep(sd, base + torch.arange(rows).view(-1, 1) * ldy + torch.arange(hs).view(1, -1), p, d)
    G = gates.view
    refs = fwd_refs(mode, o, G[:, 3 * hs:], keep, p)
    for i, name in enumerate(("r", "z", "n", "hn")):
        assert_within("%s %s" % (tag, name), G[:, i * hs:(i + 1) * hs], *refs[name])
    href, hbound = refs["h"]
    assert_within(tag + " h_out", h_out.view[:n_out], href[:n_out], hbound[:n_out])
    assert unchanged(h_out.view[n_out:]), tag + ": h_out rows past n_out changed"
    dest = (fidx.long() if fin_idx else torch.arange(rows, device=d))[n_out:]
    assert_within(tag + " h_fin", h_fin.view[dest], href[n_out:], hbound[n_out:])
    other = torch.ones(n_fin, dtype=torch.bool, device=d)
    other[dest] = False
    assert unchanged(h_fin.view[other]), tag + ": h_fin rows of unfinished sequences changed"
    if yb:
        assert_within(tag + " y", yb.view, *refs["y"])


def _ids(v):
    return str(v).replace("torch.", "")


def _n_out(sel, rows):
    return {"zero": 0, "third": rows // 3, "all": rows}[sel]


# (mode, rows, hs, in_dim, n_out, fin_idx, h_idx, y): a pairwise-covering selection -- every pair of values of two factors occurs in some
# case (in_dim: within the mode 1 cases), not the full cross product
FWD_TILE_CASES = [
    (0, 1, 64, 0, "all", False, False, None),
    (0, 127, 128, 0, "third", True, True, "plain"),
    (0, 129, 256, 0, "zero", False, True, "drop"),
    (0, 1189, 64, 0, "third", True, False, "drop"),
    (0, 1189, 128, 0, "zero", False, True, None),
    (1, 1, 128, 8, "zero", True, True, "drop"),
    (1, 127, 256, 72, "all", False, False, "drop"),
    (1, 129, 64, 128, "third", True, False, "plain"),
    (1, 129, 128, 128, "all", False, True, None),
    (1, 1189, 256, 8, "third", False, True, None),
    (1, 1189, 128, 72, "zero", True, False, "plain"),
    (1, 1189, 64, 72, "third", True, True, "drop"),
    (1, 127, 64, 8, "all", False, False, "plain"),
    (1, 129, 256, 72, "zero", True, True, None),
    (1, 1, 256, 128, "zero", False, False, "drop"),
    (1, 1189, 64, 128, "all", True, True, "drop"),
    (1, 127, 128, 128, "third", False, True, "plain"),
    (1, 129, 128, 8, "third", True, False, "drop"),
    (1, 1, 64, 72, "all", True, False, None),
    (2, 1, 256, 0, "third", True, False, "plain"),
    (2, 127, 64, 0, "zero", False, True, None),
    (2, 129, 128, 0, "all", True, True, "drop"),
    (2, 1189, 256, 0, "third", True, True, "drop"),
    (2, 1189, 64, 0, "all", False, False, "plain"),
]


@gpu
@pytest.mark.parametrize("mode,rows,hs,in_dim,n_out,fin_idx,h_idx,y", FWD_TILE_CASES)
def test_forward_single_stage_guarded(mode, rows, hs, in_dim, n_out, fin_idx, h_idx, y):
    """gru_step_fwd_kernel<0|1|2> (rows < 8192): one row, ragged panels, 10 row panels (not a multiple of the 8-way XCD interleave),
    hs of one, two and four channel tiles, a partial last k tile (in_dim 8 and 72, ldx = in_dim + 24), state rows through h_idx, finished
    rows into a column block (ld_fin = 2 hs + 8) directly and through fin_idx, y absent / ldy = 2 hs / with dropout."""
    tag = "fwd<%d> rows=%d hs=%d in=%d n_out=%s fin_idx=%d h_idx=%d y=%s" % (mode, rows, hs, in_dim, n_out, fin_idx, h_idx, y)
    run_fwd(tag, mode, rows, hs, in_dim, _n_out(n_out, rows), fin_idx, h_idx, y, seed=rows + hs + in_dim)


@gpu
@pytest.mark.parametrize("in_dim,hs", [(256, 128), (128, 256), (320, 64)])
def test_forward_pipelined_guarded(in_dim, hs):
    """gru_step_fwd_a2w3_kernel (mode 1, 8493 rows = 34 panels of 256 with a ragged last one, six 64-k stages): every output against
    float64, not only against the single-stage kernel."""
    run_fwd("fwd a2w3 in=%d hs=%d" % (in_dim, hs), 1, 8493, hs, in_dim, 8493 // 3, True, False, "drop", seed=in_dim)


@gpu
def test_forward_persistent_guarded():
    """gru_l1_fwd_persistent_kernel (mode 2, hs 256, 16461 rows = 129 row tiles over 64 workers, the last one ragged)."""
    run_fwd("fwd persistent", 2, 16461, 256, 0, 16461 // 3, True, False, None, seed=5)


# ------------------------------------------------------------------------------------------------ GPU: the fused backward step
def run_bwd(tag, rows, rows_prev, hs, dh_dtype=F32, ld_dh=None, dy=None, n_partials=None, trie=False, hprev_idx=False, hp_out=False,
            role_b=None, seed=0):
    """One gtos_gru_step_bwd(_fused) launch.  ``role_b``: (n_in, form) with form in write / acc / mask."""
    from gtos_amd._lib import call, ptr, stream
    d = dev()
    o = bwd_operands(d, rows, rows_prev, hs, seed, True, hprev_idx, trie, dh_dtype, dy is not None)
    ld_dh = hs if ld_dh is None else ld_dh
    n_ = max(rows, 1)
    dh = Guarded(n_, hs, dh_dtype, d, ld=ld_dh, init=o["dh0"])
    d4 = Guarded(n_, 4 * hs, BF, d, init=SENT)
    hpo = Guarded(n_, hs, BF, d, init=SENT) if hp_out else None
    bias0 = rnd((n_partials, 4 * hs), F32, d, seed + 20, 0.05) if n_partials else None
    bias = Guarded(n_partials, 4 * hs, F32, d, init=bias0) if n_partials else None
    ldy, p, sd, base = 2 * hs, (0.3 if dy == "drop" else 0.0), 977 + seed, 5 * 2 * hs + 8
    head = (rows, hs, ptr(o["d4_prev"]), 0 if o["rows_prev"] is None else o["rows_prev"], ptr(o["wh_t"]),
            ptr(o["gates"]) if rows else None, ptr(o["hprev"]) if rows else None, ptr(o["hprev_idx"]), ptr(o["dy"]), ldy,
            ptr(dh.view) if rows else None, 1 if dh_dtype == BF else 0, ld_dh, ptr(d4.view) if rows else None, p, sd if p > 0 else 0, base,
            None if bias is None else ptr(bias.view), n_partials or 0, None if hpo is None else ptr(hpo.view), ptr(o["sum_idx"]),
            ptr(o["dh_src"]), o["zero_row"])
    if role_b is None:
        call("gtos_gru_step_bwd", *head, stream())
    else:
        n_in, form = role_b
        ld_dinp, p_in, sd_in, base_in = n_in + 64, (0.25 if form == "mask" else 0.0), 4242, 5 * n_in
        wi_t = rnd((n_in, 3 * hs), BF, d, seed + 30, 0.1)
        old = rnd((rows_prev, n_in), BF, d, seed + 31, 0.5)
        dinp = Guarded(rows_prev, n_in, BF, d, ld=ld_dinp, init=old)
        call("gtos_gru_step_bwd_fused", *head, ptr(wi_t), ptr(dinp.view), ld_dinp, n_in, 1 if form == "acc" else 0, p_in,
             sd_in if p_in > 0 else 0, base_in, stream())
        dinp.check(tag + " dinp")                                     # the columns past n_in are band
        dp = o["d4_prev"][:, :3 * hs].double()
        ref, S = dp @ wi_t.double().t(), dp.abs() @ wi_t.double().abs().t()
        if form == "mask":
            keep = hash_keep(sd_in, base_in + torch.arange(rows_prev).view(-1, 1) * n_in + torch.arange(n_in).view(1, -1), p_in, d)
            ref, S = ref * keep * drop_scale(p_in), S * keep * drop_scale(p_in)
        if form == "acc":
            ref, S = ref + old.double(), S + old.double().abs()
        assert_bound(tag + " dinp", dinp.view, ref, S, c_acc(3 * hs), C_OUT[BF])
    for g_, w in ((dh, "dh"), (d4, "d4"), (hpo, "hp_out"), (bias, "bias partials")):
        if g_ is not None:
            g_.check(tag + " " + w)
    if rows == 0:
        assert unchanged(d4.view) and torch.equal(dh.view, o["dh0"]), tag + ": rows == 0 wrote role A outputs"
        return
    keep = None
    if p > 0:
        keep = hash_keep(sd, base + torch.arange(rows).view(-1, 1) * ldy + torch.arange(hs).view(1, -1), p, d)
    refs, hp = bwd_refs(o, keep, p, BF, dh_dtype)
    got = dict(split_d4(d4.view, hs), dh=dh.view)
    for name, (ref, bound) in refs.items():
        assert_within("%s %s" % (tag, name), got[name], ref, bound)
    if hpo is not None:
        assert torch.equal(hpo.view, hp), tag + ": hp_out is not the entering state"
    if bias is not None:
        ref, bound = bias_sum_bound(d4.view, rows)
        assert_within(tag + " bias sums", bias.view.double().sum(0) - bias0.double().sum(0), ref, bound)


# (rows, rows_prev, hs, dh dtype, ld_dh = hs + this, dy, n_partials)
BWD_A_CASES = [
    (300, 200, 64, F32, 0, None, 3),
    (300, 200, 256, BF, 64, "drop", 1024),
    (200, 300, 64, BF, 64, "plain", None),
    (200, 300, 256, F32, 0, "drop", 3),
    (1189, 1189, 64, BF, 0, "drop", 1024),
    (1189, 1189, 256, F32, 64, "plain", 3),
    (129, None, 64, F32, 64, "drop", 1024),
    (129, None, 256, BF, 0, None, 3),
]


@gpu
@pytest.mark.parametrize("rows,rows_prev,hs,dh_dtype,dh_gap,dy,n_partials", BWD_A_CASES, ids=_ids)
def test_backward_role_a_guarded(rows, rows_prev, hs, dh_dtype, dh_gap, dy, n_partials):
    """Role A of gru_step_bwd_kernel on the packed route (rows_prev given) and without a recurrent product (none): d4, dh (fp32 / bf16,
    a column block) and the bias partials (accumulated into non-zero content; 3 slots shared by many workgroups, or 1024) against the
    cell's mathematics; rows past rows_prev get no recurrent term; the last ragged panel adds nothing twice to the bias sums."""
    tag = "bwd A rows=%d prev=%s hs=%d dh=%s+%d dy=%s partials=%s" % (rows, rows_prev, hs, str(dh_dtype)[6:], dh_gap, dy, n_partials)
    run_bwd(tag, rows, rows_prev, hs, dh_dtype, hs + dh_gap, dy, n_partials, seed=rows + hs)


@gpu
@pytest.mark.parametrize("rows,hs,dh_dtype,dy,n_partials", [(300, 64, F32, "drop", 3), (300, 256, BF, None, 1024),
                                                           (1189, 64, BF, "plain", None), (129, 256, F32, "drop", 3)], ids=_ids)
def test_backward_trie_route_guarded(rows, hs, dh_dtype, dy, n_partials):
    """Role A on the trie route: operand rows and the incoming state gradient through sum_idx (a third of the rows are leaves: zero_row
    names the NaN row behind both tables, so a fetch for a leaf would show), the entering state through hprev_idx, hp_out guarded."""
    tag = "bwd trie rows=%d hs=%d dh_src=%s dy=%s partials=%s" % (rows, hs, str(dh_dtype)[6:], dy, n_partials)
    run_bwd(tag, rows, None, hs, dh_dtype, hs, dy, n_partials, trie=True, hprev_idx=True, hp_out=True, seed=rows + hs + 1)


@gpu
@pytest.mark.parametrize("rows,rows_prev,hs,n_in,form", [(300, 200, 64, 64, "write"), (200, 300, 64, 128, "acc"),
                                                         (0, 333, 256, 192, "mask"), (200, 300, 256, 192, "write"),
                                                         (300, 200, 64, 128, "mask"), (0, 129, 64, 64, "acc")])
def test_backward_role_b_guarded(rows, rows_prev, hs, n_in, form):
    """Role B (dinp = mask * d4_prev[:, 0:3hs] W_ih (+ old), ld_dinp = n_in + 64) written, accumulated and masked, alone (rows == 0)
    and beside role A with more and with fewer rows than the previous step; role A of the same launch against float64 as well."""
    tag = "bwd B rows=%d prev=%d hs=%d n_in=%d %s" % (rows, rows_prev, hs, n_in, form)
    run_bwd(tag, rows, rows_prev, hs, BF, hs, None, 3 if rows else None, role_b=(n_in, form), seed=rows + rows_prev + n_in)


# ------------------------------------------------------------------------------------------------ GPU: the unfused cells (rowops.hip)
def _cell_bwd_buffers(dtype, rows, hs, n_partials, seed):
    d = dev()
    o = bwd_operands(d, rows, None, hs, seed, True, dy=True)
    o["gates"] = guarded_operand(o["gates"].to(dtype))
    o["hprev"] = guarded_operand(o["hprev"].to(dtype))
    o["dy"] = guarded_operand(o["dy"].to(dtype), ld=2 * hs)
    dh = Guarded(rows, hs, F32, d, init=o["dh0"])
    dxg = Guarded(rows, 3 * hs, dtype, d, init=SENT)
    dhg = Guarded(rows, 3 * hs, dtype, d, init=SENT)
    bias0 = rnd((n_partials, 4 * hs), F32, d, seed + 20, 0.05) if n_partials else None
    bias = Guarded(n_partials, 4 * hs, F32, d, init=bias0) if n_partials else None
    return o, dh, dxg, dhg, bias0, bias


@gpu
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,hs,y,n_partials", [(1, 8, None, None), (1, 64, "drop", None), (1, 256, "plain", None), (37, 8, "drop", 3),
                                                  (37, 64, "plain", 3), (37, 256, "drop", 1024), (5000, 8, "plain", 1024),
                                                  (5000, 64, "drop", 3), (5000, 256, None, 3)])
def test_unfused_cells_guarded(dtype, rows, hs, y, n_partials):
    """gtos_gru_cell_fwd / gtos_gru_cell_bwd (gru_fwd_kernel / gru_bwd_kernel, the fp32 path's cells): h in place, y, the saved
    previous state and the gates; dh in place, d(xg), d(hg) and the bias partials (accumulated into non-zero content)."""
    from gtos_amd._lib import call, ptr, stream
    d, code = dev(), (1 if dtype == BF else 0)
    tag = "cell %s rows=%d hs=%d y=%s partials=%s" % (str(dtype)[6:], rows, hs, y, n_partials)
    seed = rows + hs
    xg = guarded_operand(rnd((rows, 3 * hs), dtype, d, seed + 1))
    hg = guarded_operand(rnd((rows, 3 * hs), dtype, d, seed + 2))
    h0 = rnd((rows, hs), dtype, d, seed + 3)
    h = Guarded(rows, hs, dtype, d, init=h0)
    hsave = Guarded(rows, hs, dtype, d, init=SENT)
    gates = Guarded(rows, 4 * hs, dtype, d, init=SENT)
    ldy, p, sd, base = 2 * hs, (0.3 if y == "drop" else 0.0), 31 + seed, 3 * 2 * hs + 8
    yb = Guarded(rows, hs, dtype, d, ld=ldy, init=SENT) if y else None
    call("gtos_gru_cell_fwd", code, rows, hs, ptr(xg), ptr(hg), ptr(h.view), None if yb is None else ptr(yb.view), ldy, ptr(hsave.view),
         ptr(gates.view), p, sd if p > 0 else 0, base, stream())
    for g_, w in ((h, "h"), (hsave, "hprev_save"), (gates, "gates")) + (((yb, "y"),) if yb else ()):
        g_.check(tag + " " + w)
    idx = base + torch.arange(rows).view(-1, 1) * ldy + torch.arange(hs).view(1, -1)
    keep = hash_keep(sd, idx, p, d) if p > 0 else None
    G = gates.view
    refs = gru_fwd_bounds(xg.double(), xg.double().abs(), hg.double(), hg.double().abs(), h0.double(), G[:, 3 * hs:], 1, dtype, keep, p)
    for i, name in enumerate(("r", "z", "n", "hn")):
        assert_within("%s %s" % (tag, name), G[:, i * hs:(i + 1) * hs], *refs[name])
    assert torch.equal(G[:, 3 * hs:], hg[:, 2 * hs:]) and torch.equal(hsave.view, h0), tag + ": hn / hprev_save are copies"
    assert_within(tag + " h", h.view, *refs["h"])
    if yb:
        assert_within(tag + " y", yb.view, *refs["y"])
    # backward
    o, dh, dxg, dhg, bias0, bias = _cell_bwd_buffers(dtype, rows, hs, n_partials, seed + 40)
    dy = o["dy"] if y else None
    call("gtos_gru_cell_bwd", code, rows, hs, ptr(o["gates"]), ptr(o["hprev"]), ptr(dy), ldy, ptr(dh.view), ptr(dxg.view), ptr(dhg.view),
         p, sd if p > 0 else 0, base, None if bias is None else ptr(bias.view), n_partials or 0, stream())
    for g_, w in ((dh, "dh"), (dxg, "dxg"), (dhg, "dhg"), (bias, "bias partials")):
        if g_ is not None:
            g_.check(tag + " " + w)
    if dy is None:
        o["dy"] = None
    refs, _ = bwd_refs(o, keep, p, dtype, F32)
    got = dict(split_d4(torch.cat([dxg.view, dhg.view[:, 2 * hs:]], 1), hs), dh=dh.view)
    for name, (ref, bound) in refs.items():
        assert_within("%s %s" % (tag, name), got[name], ref, bound)
    assert torch.equal(dhg.view[:, :2 * hs], dxg.view[:, :2 * hs]), tag + ": d(hg) r, z blocks"
    if bias is not None:
        ref, bound = bias_sum_bound(torch.cat([dxg.view, dhg.view[:, 2 * hs:]], 1), rows)
        assert_within(tag + " bias sums", bias.view.double().sum(0) - bias0.double().sum(0), ref, bound)


@gpu
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_unfused_backward_refuses_bias_sums_it_cannot_own(dtype):
    """hs = 24: a thread would not keep its 8 channels over its grid-stride rows (256 % (hs / 8) != 0): with bias partials the entry point
    returns -26 and launches nothing -- every buffer, views included, keeps its content."""
    from gtos_amd._lib import GtosHipError, call, ptr, stream
    rows, hs, n_partials = 37, 24, 3
    o, dh, dxg, dhg, bias0, bias = _cell_bwd_buffers(dtype, rows, hs, n_partials, 7)
    with pytest.raises(GtosHipError, match="code -26"):
        call("gtos_gru_cell_bwd", 1 if dtype == BF else 0, rows, hs, ptr(o["gates"]), ptr(o["hprev"]), ptr(o["dy"]), 2 * hs, ptr(dh.view),
             ptr(dxg.view), ptr(dhg.view), 0.0, 0, 0, ptr(bias.view), n_partials, stream())
    for g_, w in ((dh, "dh"), (dxg, "dxg"), (dhg, "dhg"), (bias, "bias partials")):
        g_.check("refused cell bwd " + w)
    assert torch.equal(dh.view, o["dh0"]) and unchanged(dxg.view) and unchanged(dhg.view) and torch.equal(bias.view, bias0)
