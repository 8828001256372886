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
_INT_OF = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}


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
