"""Shared constants (must match tests/golden/make_golden.py) and helpers of the tests."""
import ctypes
import os
import subprocess

import torch

SMALL_VOCAB = dict(concept=60, token=70, predictable_token=50, relation=26, concept_char=20, token_char=22)
SMALL_GEN_ARGS = (8, 12, 8, 12, [(3, 16)], 10, 10, 6, 8, 2)   # char/word dims, filters, rel_dim, rnn


def compile_host_driver(tmp_path_factory, name, source):
    """``source`` (C++ that includes rule headers of gtos_amd/csrc and exports extern "C" functions) compiled with $CXX (g++) as the
    kernels' exact-FP objects are (no contraction) -> the loaded ctypes.CDLL.  ``name``: of the temporary directory and the library."""
    d = tmp_path_factory.mktemp(name)
    src, lib = d / "driver.cpp", d / ("lib%s.so" % name)
    src.write_text(source)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                           "-I", os.path.join(root, "gtos_amd", "csrc"), str(src), "-o", str(lib)])
    return ctypes.CDLL(str(lib))


def full_model_pair(dev, cfg_name, B, layers=None):
    """Product Generator on the GPU and the pinned oracle on the CPU with identical weights (train.sh dims, dropout 0)."""
    from gtos_amd import synth
    from gtos_amd.config import default_vocabs, generator_args
    from gtos_amd.generator import Generator
    from oracle import gtos_oracle as O
    cfg = dict(synth.CONFIGS[cfg_name])
    if layers:
        cfg["layers"] = layers
    args = generator_args(cfg)
    args["dropout"] = 0.0
    depth = 256 if cfg["kind"] == "dep" else 32
    torch.manual_seed(11)
    ref = O.Generator({k: O.VocabSpec(v.size, 0) for k, v in default_vocabs().items()}, depth_size=depth, **args)
    for p in ref.parameters():
        if p.dim() == 1 or float(p.detach().abs().sum()) == 0:
            p.data.add_(0.02 * torch.randn_like(p))
    m = Generator(default_vocabs(), device=dev, depth_size=depth, **args).to(dev)
    m.load_state_dict(ref.state_dict())
    batch, stats = synth.make_config_batch(cfg_name, B=B, padded=True)
    return ref, m, batch, stats


# ------------------------------------------------------------------------------------------------ guard bands
# A kernel output carved from the middle of one larger allocation: `lead` rows of band in front, a gap of columns between the view's
# width and its leading dimension, `trail` rows of band behind (and, with `shift`, a few elements in front of the first row that
# misalign its base).  Everything outside the view holds a fixed NaN bit pattern; after the launch the bands are compared BITWISE, so a
# store one row or column too many is found whatever it wrote.  The default bands hold a full 256x256 macro tile of rows past the end:
# a ragged tile that stores rows it should not lands inside the band, never past the allocation.
NAN_BITS = {torch.float32: 0x7FC0A5A5, torch.bfloat16: 0x7FC5}
_INT_OF = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64, torch.uint8: torch.uint8,
           torch.int64: torch.int64}


def _bits(t):
    return t.view(_INT_OF[t.dtype])


class Guarded:
    """``Guarded(rows, cols, dtype, device, ld=, lead=, trail=, shift=, init=)``: ``.view`` is the [rows, cols] tensor (row stride ld);
    ``.check(what)`` asserts that no element outside it changed.  ``init`` (a tensor or a number) fills the view; the rest of the
    allocation holds the NaN pattern of the dtype (``band`` overrides it: an int bit pattern)."""

    def __init__(self, rows, cols, dtype, device, ld=None, lead=256, trail=256, shift=0, init=None, band=None):
        ld = cols if ld is None else ld
        assert ld >= cols and shift >= 0
        self._setup(rows, cols, ld, lead * ld + shift, lead * ld + shift + (rows + trail) * ld, dtype, device, init, band)

    def _setup(self, rows, cols, ld, base, total, dtype, device, init, band):
        self.rows, self.cols, self.ld, self.base, self.dtype = rows, cols, ld, base, dtype
        self.buf = torch.empty(total, dtype=dtype, device=device)
        self.pattern = NAN_BITS[dtype] if band is None else band
        _bits(self.buf).fill_(self.pattern)
        self.regions = []
        self.view = self.carve(base, rows, cols, ld, init)

    def carve(self, offset, rows, cols, ld, init=None):
        """One more [rows, cols] view (row stride ld) starting ``offset`` elements into the allocation; every region carved is exempt
        from the band check (several outputs of one launch, back to back in one buffer)."""
        assert offset >= 0 and offset + (rows - 1) * ld + cols <= self.buf.numel()
        self.regions.append((offset, rows, cols, ld))
        v = self.buf.as_strided((rows, cols), (ld, 1), offset)
        if isinstance(init, torch.Tensor):
            v.copy_(init.reshape(rows, cols))
        elif init is not None:
            v.fill_(init)
        return v

    def band_mask(self):
        inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        for off, rows, cols, ld in self.regions:
            inside.as_strided((rows, cols), (ld, 1), off).fill_(True)
        return ~inside

    def check(self, what=""):
        if self.buf.is_cuda:
            torch.cuda.synchronize()
        bad = (_bits(self.buf) != self.pattern) & self.band_mask()
        n = int(bad.sum())
        if n:
            idx = torch.nonzero(bad).flatten()[:8].tolist()
            ld = max(self.ld, 1)
            where = ["element %d (row %d col %d of the view's grid)" % (i, (i - self.base) // ld, (i - self.base) % ld) for i in idx]
            raise AssertionError("%s: %d element(s) outside the [%d x %d, ld %d] view changed, first at %s" % (
                what, n, self.rows, self.cols, self.ld, ", ".join(where)))


class GuardedFlat(Guarded):
    """A 1-D output of n elements with ``lead`` / ``trail`` band elements around it (``.view`` is 1-D)."""

    def __init__(self, n, dtype, device, lead=1024, trail=1024, init=None, band=None):
        self._setup(1, n, n, lead, lead + n + trail, dtype, device, init, band)
        self.view = self.view[0]


def nan_buffer(n, dtype, device):
    """A band-only allocation of n elements: carve() the outputs of one launch out of it, then check() the rest."""
    g = GuardedFlat(0, dtype, device, lead=n, trail=0)
    g.regions = []
    return g


def guarded_operand(t, ld=None, shift=0, lead=8, trail=8):
    """An INPUT operand equal to ``t`` (2-D) whose leading-dimension gap and surrounding rows hold NaN: a kernel that reads past the
    operand's columns multiplies NaN into its result instead of finite data that a zero in the other operand would hide."""
    g = Guarded(t.shape[0], t.shape[1], t.dtype, t.device, ld=ld, lead=lead, trail=trail, shift=shift, init=t)
    return g.view


# Products against float64: |got - ref| <= c_acc * S + c_out * |ref|, S = |A| @ |B| (+ |bias| + |C0|): the rounding error of an fp32
# accumulation of K terms is a multiple of fp32 epsilon times S (the bf16 products themselves are exact in fp32), and a bf16 output
# adds half an ulp of the result.  c_acc = 4 eps sqrt(K) sits far above the probabilistic rounding error of a blocked sum and far
# below one typical product term (the self-check in tests/test_guard_bands.py shows it rejects one dropped k term).
EPS32 = 2.0 ** -23


def c_acc(K):
    return 4.0 * EPS32 * max(1.0, float(K)) ** 0.5


C_OUT = {torch.float32: EPS32, torch.bfloat16: 2.0 ** -8}


def bound_ratio(got, ref, S, cacc, cout, extra=None):
    """max over elements of |got - ref| / (cacc * S + cout * |ref| + extra) (NaN anywhere -> inf); <= 1 passes."""
    got = got.double()
    err = (got - ref).abs()
    bound = cacc * S + cout * ref.abs() + (0 if extra is None else extra) + 1e-30
    r = err / bound
    if bool(torch.isnan(r).any()):
        return float("inf"), float("nan")
    return float(r.max()), float(err.max())


def assert_bound(name, got, ref, S, cacc, cout, extra=None):
    ratio, err = bound_ratio(got, ref, S, cacc, cout, extra)
    print("MEASURED %s: max |err| %.3e, max err/bound %.3e (c_acc %.2e, c_out %.2e)" % (name, err, ratio, cacc, cout))
    assert ratio <= 1.0, "%s: error %.3e exceeds the bound by %.2fx" % (name, err, ratio)


# ------------------------------------------------------------------------------------------------ GRU step kernels: fp64 and bounds
# The step kernels (csrc/gru_step.hip, the unfused cells of csrc/rowops.hip) against float64 restatements of one time step, every error
# propagated to first order from three constants and no free tolerance:
#   c_acc(K) * S     an fp32 accumulation of K terms whose absolute values sum to S (products, bias and elementwise additions),
#   C_OUT[dtype]     half an ulp of a stored output, relative to its value,
#   c_fast(pre)      __expf / v_rcp_f32 behind a sigmoid or the fast tanh: 1-ulp hardware exp2 and rcp plus the rounding of the scaled
#                    argument, which grows with the pre-activation: 32 eps (1 + |pre|).
# With u the first-order error of a value BEFORE it is rounded to its stored type, the stored value is held to
# C_OUT |ref| + (1 + C_OUT) u: the half ulp is taken of the computed value, which may exceed |ref| by u.
def c_fast(pre):
    return 32.0 * EPS32 * (1.0 + pre.abs())


def within_ratio(got, ref, bound):
    """max over elements of |got - ref| / bound (NaN anywhere -> inf) and the largest error"""
    err = (got.double() - ref).abs()
    r = err / (bound + 1e-30)
    if bool(torch.isnan(r).any()):
        return float("inf"), float("nan")
    if r.numel() == 0:
        return 0.0, 0.0
    return float(r.max()), float(err.max())


def assert_within(name, got, ref, bound):
    ratio, err = within_ratio(got, ref, bound)
    print("MEASURED %s: max |err| %.3e, max err/bound %.3e" % (name, err, ratio))
    assert ratio <= 1.0, "%s: error %.3e exceeds the bound by %.2fx" % (name, err, ratio)


def stored_bound(ref, u, dtype):
    return C_OUT[dtype] * ref.abs() + (1.0 + C_OUT[dtype]) * u


def drop_scale(p):
    """1 / (1 - p) of the fp32 p the kernels are handed"""
    return 1.0 / (1.0 - float(torch.tensor(p, dtype=torch.float32))) if p > 0 else 1.0


def gru_fwd_bounds(xg, Sx, hg, Sh, h, hn_stored, K, dtype, keep=None, p=0.0):
    """One forward step in float64.  ``xg`` / ``hg`` [rows, 3hs]: the input and recurrent gate pre-activations WITH their biases, from the
    stored operands; ``Sx`` / ``Sh``: the same sums over absolute values; ``h`` [rows, hs]: the entering state; ``hn_stored``: the
    kernel's own stored hn = hg_n (the kernel rounds it to the stored type before it uses it, for backward's sake: n and h' are
    restated from that value, hn itself is held to the fp64 product); ``K``: terms per pre-activation; ``keep``: the dropout mask of y.
    Returns {name: (ref, bound)} for r, z, hn, n, h, y -- the bounds are those of values stored as ``dtype``."""
    hs = h.shape[1]
    ca = c_acc(K)

    def blk(t, g):
        return t[:, g * hs:(g + 1) * hs]
    ref, u = {}, {}
    for g, name in enumerate("rz"):
        pre = blk(xg, g) + blk(hg, g)
        ref[name] = torch.sigmoid(pre)
        u[name] = ca * (blk(Sx, g) + blk(Sh, g)) / 4 + c_fast(pre)            # |sigmoid'| <= 1/4
    ref["hn"], u["hn"] = blk(hg, 2), ca * blk(Sh, 2)
    hn = hn_stored.double()
    r, z = ref["r"], ref["z"]
    pre_n = blk(xg, 2) + r * hn
    n = ref["n"] = torch.tanh(pre_n)
    u["n"] = ca * (blk(Sx, 2) + (r * hn).abs()) + hn.abs() * u["r"] + c_fast(pre_n)          # |tanh'| <= 1
    ref["h"] = (1 - z) * n + z * h
    u["h"] = u["z"] * (h - n).abs() + (1 - z) * u["n"] + c_acc(1) * (((1 - z) * n).abs() + (z * h).abs())
    ks = drop_scale(p)
    keep = torch.ones_like(h) if keep is None else keep.double()
    ref["y"] = keep * ref["h"] * ks
    u["y"] = keep * ks * u["h"] + c_acc(1) * ref["y"].abs()                    # 1 / (1 - p) and the product in fp32
    return {k: (ref[k], stored_bound(ref[k], u[k], dtype)) for k in ref}


def gru_bwd_bounds(gates, hp, g_in, S_in, P, S_P, K, d4_dtype, dh_dtype):
    """One backward step of the cell in float64.  ``gates`` [rows, 4hs] = (r | z | n | hn) and ``hp`` [rows, hs] as stored;
    ``g_in`` = dh + drop(dy) and ``S_in`` = |dh| + |drop(dy)|; ``P`` / ``S_P``: the recurrent product
    d4_prev[src][:, {0:2hs, 3hs:4hs}] @ wh_t^T and its sum over absolute values (zero rows where there is none); ``K`` its depth.
    The error of g = g_in + P, c_acc(K) (S_in + S_P), reaches every output times the elementwise factor that multiplies g; the factors
    are exact functions of stored values up to fp32 roundings (8 eps of the result; 1 - n^2 cancels: eps n^2 absolute).
    Returns {name: (ref, bound)} for dr, dz, dn, dhn (the four blocks of d4) and dh (= g z)."""
    hs = hp.shape[1]
    gr, gz, gn, hn = (gates[:, i * hs:(i + 1) * hs].double() for i in range(4))
    hp = hp.double()
    g = g_in + P
    e_g = c_acc(K) * (S_in + S_P)
    q = 1 - gn * gn
    fac = {"dn": (1 - gz) * q, "dz": (hp - gn) * gz * (1 - gz), "dh": gz}
    fac["dhn"] = fac["dn"] * gr
    fac["dr"] = fac["dn"] * hn * gr * (1 - gr)
    noq = {"dn": (1 - gz), "dhn": (1 - gz) * gr, "dr": (1 - gz) * hn * gr * (1 - gr)}     # the factor without 1 - n^2
    out = {}
    for k, f in fac.items():
        ref = g * f
        u = e_g * f.abs() + 8 * EPS32 * ref.abs()
        if k in noq:
            u = u + EPS32 * gn * gn * (g * noq[k]).abs()
        out[k] = (ref, stored_bound(ref, u, dh_dtype if k == "dh" else d4_dtype))
    return out


def bias_sum_bound(d4_stored, rows):
    """(fp64 column sums of the stored d4 rows, c_acc(rows) * column sums of |d4|)"""
    d = d4_stored.double()
    return d.sum(0), c_acc(rows) * d.abs().sum(0)


# ------------------------------------------------------------------------------------------------ row kernels: fp64 and bounds
# The gather / scatter / elementwise row kernels (csrc/tokenenc.hip, the middle of csrc/rowops.hip) against float64, with the same three
# constants.  Where a kernel only moves or selects stored values the tests ask for equality; the functions below are for the rest.
def c_acc_of(count):
    """c_acc of a tensor of term counts (a count of 0 or 1 is one rounding)"""
    return 4.0 * EPS32 * count.double().clamp(min=1.0).sqrt()


def highway_bounds(y, x, dout, dtype):
    """The highway gate of csrc/tokenenc.hip.  ``y`` [N, 2D] = (new_x | gate), ``x``, ``dout`` [N, D] as stored.  The sigmoid's error
    c_fast(gate) reaches every output times the magnitude it multiplies; the fp32 products and sums add c_acc(1) of the terms (8 eps
    for the four-factor product of dg).  relu and its gate are exact: dnx is 0 with no error wherever new_x <= 0.
    Returns {name: (ref, bound)} for out, dnx, dg, dx."""
    D = x.shape[1]
    nx, g, x, go = y[:, :D].double(), y[:, D:].double(), x.double(), dout.double()
    s, r, cf = torch.sigmoid(g), nx.clamp(min=0.0), c_fast(g)
    on = (nx > 0).double()
    ref = dict(out=s * x + (1 - s) * r, dnx=on * go * (1 - s), dg=go * (x - r) * s * (1 - s), dx=go * s)
    u = dict(out=cf * (x - r).abs() + c_acc(1) * ((s * x).abs() + ((1 - s) * r).abs()),
             dnx=on * (cf * go.abs() + c_acc(1) * ref["dnx"].abs()),
             dg=cf * (go * (x - r)).abs() + 8 * EPS32 * ref["dg"].abs(),
             dx=cf * go.abs() + c_acc(1) * ref["dx"].abs())
    return {k: (ref[k], stored_bound(ref[k], u[k], dtype)) for k in ref}


def dropped_rows_bounds(val, keep, p, dtype):
    """Rows of stored values ``val`` (float64) through dropout: kept elements val / (1 - p) in fp32 (the quotient and the product:
    c_acc(1) of the result) rounded to ``dtype``, dropped elements exactly 0 (bound 0).  p == 0: one rounding of val."""
    ref = val * keep.double() * drop_scale(p) if p > 0 else val
    return ref, stored_bound(ref, c_acc(1) * ref.abs() if p > 0 else torch.zeros_like(ref), dtype)


def scatter_bounds(pre, tok, v):
    """table[tok[n], :] += v[n, :] on top of the preload ``pre`` (fp32 atomics in any order).  ``v`` float64 [n, C].  Returns (ref, bound,
    count): per element c_acc(count) * S with count the rows that share the token and S = |pre| + sum |v|.  A row with count 0 has to
    stay bitwise what it was: the callers check that apart."""
    tok = tok.long()
    ref = pre.double().index_add(0, tok, v)
    S = pre.double().abs().index_add(0, tok, v.abs())
    count = torch.bincount(tok, minlength=pre.shape[0])
    return ref, c_acc_of(count)[:, None] * S, count


def gather_mean_bounds(bank, idx, dtype):
    """out[p] = mean over the live (non-zero) entries of idx[p] of bank rows, row 0 never read.  Bound: c_acc(K) * S / cnt (the sum, the
    reciprocal and the product) plus the stored rounding."""
    b = bank.double().clone()
    b[0] = 0.0
    live = (idx != 0)
    rows = b[idx.long()] * live.double()[..., None]
    cnt = live.sum(1).clamp(min=1).double()[:, None]
    ref = rows.sum(1) / cnt
    return ref, stored_bound(ref, c_acc(idx.shape[1]) * rows.abs().sum(1) / cnt, dtype)


def segment_sum_bounds(v, node_of_row, n_nodes, dtype=torch.bfloat16):
    """dst[node] = sum of the node's rows ``v`` (float64 [rows, W]), fp32 accumulation in any order, one rounding to ``dtype``:
    c_acc(cnt) * S per element with cnt the NODE's row count, so a two-row node is held to its own error.  Empty nodes: exactly 0."""
    ref = torch.zeros(n_nodes, v.shape[1], dtype=torch.float64, device=v.device).index_add(0, node_of_row, v)
    S = torch.zeros_like(ref).index_add(0, node_of_row, v.abs())
    cnt = torch.bincount(node_of_row, minlength=n_nodes)
    return ref, stored_bound(ref, c_acc_of(cnt)[:, None] * S, dtype)


# ------------------------------------------------------------------------------------------------ relation attention: fp64 and bounds
# The streaming attention kernels (csrc/rel_attn.hip: forward, query-major and key-major backward, bank gradient) against a float64
# restatement on the stored operands, every error propagated to first order from the same three constants:
#   c_acc(K) * S     every fp32 sum (a score over the hd channels of a head, the softmax denominator, o / dq over the keys, dk / dv over
#                    the queries, a bank row over the pairs of its type -- fp32 atomics in any order for a heavy type: a sum's rounding
#                    error does not depend on its order to first order, so the same c_acc(count) holds),
#   C_OUT[dtype]     a stored value (stored_bound),
#   c_fast(x)        __expf (exp2 of a scaled argument: the argument's rounding grows with |x|), the reciprocal 1 / l (c_fast(0)) and
#                    __logf = log2(l) * ln 2 (c_fast(log l), an ABSOLUTE error: one ulp of the hardware log2's result, the product with
#                    ln 2, and a floor of 32 eps where log l is near zero).  c_fast was defined for 1-ulp hardware exp2 and rcp;
#                    v_log_f32 is a 1-ulp transcendental of the same unit (kernel guide, cdna_hip_programming.md Guideline 8 "Use
#                    appropriate math precision and intrinsics", and the transcendental row of MI355X_MICROARCH.md's issue-cost table),
#                    so no further constant is needed.
# Softmax.  With e_s the error of a score, p_j = exp(s_j) / sum_k exp(s_k) moves by p_j (ds_j - sum_k p_k ds_k) <= p_j (e_s_j + E),
# E = sum_k p_k e_s_k.  The kernels rescale running sums by exp(m_old - m_new) each time the maximum grows and when lanes and waves are
# merged: a term reaches the final sum through at most nf = ceil(S / KS) + log2(G) + 4 factors __expf(a_k) whose arguments add up to
# m - s_j = delta_j, so its relative error is sum_k c_fast(a_k) = nf * c_fast(delta_j / nf) = r_j.  The denominator adds c_acc(S) and
# the reciprocal c_fast(0).
# Backward.  The kernels read the STORED o (D = sum d_o o + sum w dw) and the STORED lse (p = exp(s - lse)) and w: their bounds from the
# forward enter D and p as operand errors.  pd (the weights the key-major pass multiplies into dv) is p keep / (1 - p_drop) from that p,
# or, when the forward returned w, w itself.  In bf16 the half ulp of o is the largest term of the whole backward: D moves by up to
# 2^-8 sum |d_o| |o|, and every gs_ij by scale p_ij times that.
def lse_comparable(got, ref):
    """(got, ref) with the -inf entries of ref (fully masked rows) replaced: 0 where got is -inf as well, NaN (-> ratio inf) where not"""
    dead = torch.isinf(ref)
    g = torch.where(dead, torch.where(got.double() == ref, 0.0, float("nan")), got.double())
    return g, torch.where(dead, torch.zeros_like(ref), ref)


def rel_attn_ref(q, k, v, H, scale, mode=0, rel=None, ids=None, R=None, key_pad=None, attn_mask=None, p_drop=0.0, keep=None,
                 d_o=None, d_w=None):
    """float64 relation attention on the stored operands.  q [T,B,d], k / v [S,B,d]; mode 1: rel = rarb [S,T,B,2d] (key-major);
    mode 2: rel = bank [>=R,2d] and ids [S,T,B] = relation[j,i,b] (bit 31 ignored); key_pad [S,B], attn_mask [T,S] (non-zero = masked);
    keep [T,S,B,H] bool (the restated drop_keep) when p_drop > 0; d_o [T,B,d], d_w [T,S,B,H] or None.
    Returns a dict: o, lse (-inf on fully masked rows), w, and with d_o: pd, gs, dq, dk, dv, d_rel (mode 1: [S,T,B,2d]; mode 2: [R,2d],
    zero rows for types without pairs) -- plus the intermediates rel_attn_bounds needs (keys starting with '_')."""
    T, B, d = q.shape
    S, hd = k.shape[0], d // H
    q5, k5 = q.double().reshape(T, 1, B, H, hd), k.double().reshape(1, S, B, H, hd)
    v4 = v.double().reshape(S, B, H, hd)
    full = (T, S, B, H, hd)
    if mode == 0:
        qa, kb, qa_abs, kb_abs = q5.expand(full), k5.expand(full), q5.abs().expand(full), k5.abs().expand(full)
    else:
        rows = rel.double() if mode == 1 else rel.double()[ids.long() & 0x7fffffff]
        rows = rows.reshape(S, T, B, 2 * d).permute(1, 0, 2, 3)
        ra, rb = rows[..., :d].reshape(full), rows[..., d:].reshape(full)
        qa, kb, qa_abs, kb_abs = q5 + ra, k5 + rb, q5.abs() + ra.abs(), k5.abs() + rb.abs()
    s = scale * (qa * kb).sum(-1)
    s_abs = abs(scale) * (qa_abs * kb_abs).sum(-1)
    dead = torch.zeros(T, S, B, 1, dtype=torch.bool, device=q.device)
    if key_pad is not None:
        dead = dead | (key_pad != 0).reshape(1, S, B, 1)
    if attn_mask is not None:
        dead = dead | (attn_mask != 0).reshape(T, S, 1, 1)
    dead = dead.expand(T, S, B, H)
    sm = s.masked_fill(dead, float("-inf"))
    m = sm.amax(1, keepdim=True)
    has = torch.isfinite(m)
    m0 = torch.where(has, m, torch.zeros_like(m))
    e = torch.exp(sm - m0)
    l = e.sum(1, keepdim=True)
    p = e / l.clamp_min(1e-300)
    logl = torch.log(l.clamp_min(1e-300)) * has
    lse = torch.where(has, m0 + logl, torch.full_like(m, float("-inf"))).squeeze(1)
    kf = keep.double() * drop_scale(p_drop) if p_drop > 0 else torch.ones_like(p)
    w = kf * p
    o = torch.einsum("ijbh,jbhe->ibhe", w, v4).reshape(T, B, d)
    out = dict(o=o, lse=lse, w=w, _p=p, _kf=kf, _s_abs=s_abs, _delta=torch.where(dead, torch.zeros_like(s), m0 - s), _logl=logl,
               _m=m0, _v4=v4, _qa_abs=qa_abs, _kb_abs=kb_abs, _dims=(T, S, B, H, hd, mode), _dead=dead)
    if d_o is None:
        return out
    do4 = d_o.double().reshape(T, B, H, hd)
    dw = torch.zeros_like(w) if d_w is None else d_w.double()
    D = (do4 * o.reshape(T, B, H, hd)).sum(-1) + (w * dw).sum(1)
    dpv = torch.einsum("ibhe,jbhe->ijbh", do4, v4)
    X = kf * (dpv + dw) - D[:, None]
    gs = scale * p * X
    out.update(pd=w, gs=gs, dq=torch.einsum("ijbh,ijbhe->ibhe", gs, kb).reshape(T, B, d),
               dk=torch.einsum("ijbh,ijbhe->jbhe", gs, qa).reshape(S, B, d), dv=torch.einsum("ijbh,ibhe->jbhe", w, do4).reshape(S, B, d),
               _do4=do4, _dw=dw, _D=D, _dpv=dpv, _X=X, _scale=abs(scale))
    if mode:
        pair = torch.cat([(gs[..., None] * kb).reshape(T, S, B, d), (gs[..., None] * qa).reshape(T, S, B, d)], -1).permute(1, 0, 2, 3)
        if mode == 1:
            out["d_rel"] = pair
        else:
            tid = (ids.long() & 0x7fffffff).reshape(-1)
            out["d_rel"] = torch.zeros(R, 2 * d, dtype=torch.float64, device=q.device).index_add_(0, tid, pair.reshape(-1, 2 * d))
            out["_tid"], out["_R"] = tid, R
    return out


def rel_attn_bounds(ref, dtype, KS, G, with_w=False):
    """{name: elementwise bound} for every output of ``rel_attn_ref`` stored as ``dtype`` (o, dq, dk, dv, d_rel; lse, w, pd, gs are fp32).
    KS = 4 G: the keys a workgroup takes per step, G the key groups of a wave (the kernels' geometry): they set the length nf of the
    longest chain of rescaling factors.  The bound of lse is that of its finite entries (0 where the reference is -inf).
    ``with_w``: the backward is handed the forward's w, and its pd is then that tensor (and carries its bound)."""
    T, S, B, H, hd, mode = ref["_dims"]
    F32 = torch.float32
    p, kf, w = ref["_p"], ref["_kf"], ref["w"]
    nf = -(-S // KS) + max(G, 1).bit_length() - 1 + 4
    e_s = c_acc(hd) * ref["_s_abs"]
    r = nf * c_fast(ref["_delta"] / nf)
    rel_l = (p * (e_s + r)).sum(1, keepdim=True) + c_acc(S)
    u_p = p * (e_s + r + rel_l + c_fast(torch.zeros(())))
    u_w = kf * u_p + c_acc(1) * w
    v_abs = ref["_v4"].abs()
    u_o = (torch.einsum("ijbh,jbhe->ibhe", u_w, v_abs) + c_acc(S) * torch.einsum("ijbh,jbhe->ibhe", w, v_abs)).reshape(T, B, H * hd)
    logl, m = ref["_logl"], ref["_m"]
    u_lse = (rel_l + c_fast(logl) + c_acc(1) * (m.abs() + logl.abs())).squeeze(1)
    lse_fin = torch.where(torch.isinf(ref["lse"]), torch.zeros_like(ref["lse"]), ref["lse"])
    b = dict(o=stored_bound(ref["o"], u_o, dtype), w=stored_bound(w, u_w, F32),
             lse=stored_bound(lse_fin, u_lse, F32) * torch.isfinite(ref["lse"]))
    if "gs" not in ref:
        return b
    do_abs, dw_abs, D, X, gs, scale = ref["_do4"].abs(), ref["_dw"].abs(), ref["_D"], ref["_X"], ref["gs"], ref["_scale"]
    o4 = ref["o"].reshape(T, B, H, hd)
    u_D = ((do_abs * b["o"].reshape(T, B, H, hd)).sum(-1) + c_acc(hd) * (do_abs * o4.abs()).sum(-1)
           + (b["w"] * dw_abs).sum(1) + c_acc(S) * (w * dw_abs).sum(1) + c_acc(1) * D.abs())
    u_pb = p * (e_s + b["lse"][:, None] + c_fast(ref["_delta"] + logl))            # p again, from the stored lse
    u_pd = u_w if with_w else kf * u_pb + c_acc(1) * w
    dpv = ref["_dpv"]
    u_X = (kf * (c_acc(hd) * torch.einsum("ibhe,jbhe->ijbh", do_abs, v_abs) + c_acc(1) * (dpv.abs() + dw_abs))
           + u_D[:, None] + c_acc(1) * (kf * (dpv + ref["_dw"]).abs() + D.abs()[:, None]))
    u_gs = scale * (u_pb * X.abs() + p * u_X) + c_acc(1) * gs.abs()
    qa_abs, kb_abs, g_abs = ref["_qa_abs"], ref["_kb_abs"], gs.abs()
    d = H * hd
    u_dq = torch.einsum("ijbh,ijbhe->ibhe", u_gs + c_acc(S) * g_abs, kb_abs).reshape(T, B, d)
    u_dk = torch.einsum("ijbh,ijbhe->jbhe", u_gs + c_acc(T) * g_abs, qa_abs).reshape(S, B, d)
    u_dv = torch.einsum("ijbh,ibhe->jbhe", u_pd + c_acc(T) * w, do_abs).reshape(S, B, d)
    b.update(pd=stored_bound(w, u_pd, F32), gs=stored_bound(gs, u_gs, F32), dq=stored_bound(ref["dq"], u_dq, dtype),
             dk=stored_bound(ref["dk"], u_dk, dtype), dv=stored_bound(ref["dv"], u_dv, dtype))
    if mode:
        def halves(x):
            return torch.cat([(x[..., None] * kb_abs).reshape(T, S, B, d), (x[..., None] * qa_abs).reshape(T, S, B, d)], -1).permute(1, 0, 2, 3)
        if mode == 1:
            b["d_rel"] = stored_bound(ref["d_rel"], halves(u_gs + c_acc(1) * g_abs), dtype)
        else:
            tid, R = ref["_tid"], ref["_R"]
            zero = torch.zeros(R, 2 * d, dtype=torch.float64, device=gs.device)
            U = zero.clone().index_add_(0, tid, halves(u_gs).reshape(-1, 2 * d))
            Sabs = zero.index_add_(0, tid, halves(g_abs).reshape(-1, 2 * d))
            cnt = torch.bincount(tid, minlength=R)[:R]
            b["d_rel"] = stored_bound(ref["d_rel"], U + c_acc_of(2 * cnt)[:, None] * Sabs, dtype)      # per pair: gs k and gs RB
    return b
