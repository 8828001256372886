"""The row gather, scatter and elementwise kernels one at a time, against float64, inside guard bands.

csrc/tokenenc.hip holds the highway gate, max-over-time + relu and the token row assembly (each with its backward); the middle of
csrc/rowops.hip holds the relation gather-mean, the label-embedding rows (forward, packed-path forward, backward with embed_reduce_kernel)
and the segmented sums (seg_sum_kernel<SLABS,NSRC>, seg_sum_stream_kernel<SLABS,HALF>, seg_sum_range_kernel<SLABS>, seg_finish_kernel).
Every GPU case launches ONE of them through its C entry point with all outputs carved from NaN-filled allocations
(tests_support.Guarded: bands compared bitwise) and pre-filled with a sentinel, all 2-D inputs with NaN around their rows and in their
leading-dimension gap where the entry point takes one, and holds every element of every output to a float64 restatement from the stored
operands: equality where the kernel only moves or selects stored values, first-order bounds from c_acc, C_OUT, c_fast and stored_bound
(tests_support.highway_bounds, dropped_rows_bounds, scatter_bounds, gather_mean_bounds, segment_sum_bounds) elsewhere.  Dropout masks
are predicted with the numpy restatement of drop_keep at the counter each kernel documents (row * Cp + column, row * dim_pad + column).

Which case reaches which branch:
  grid-stride kernels (tokenenc.hip, gather_mean, embed_rows_fwd, embed_packed_paths): grids are capped at 8192 blocks of 256 threads,
      one thread per 8 channels: a case with more than 2 097 152 work items takes the second lap (the "second lap" cases).
  gtos_embed_rows_bwd: V * dim_pad * 4 <= 60 KiB -> private LDS table, else global atomics; LDS with a workspace and more than 8 blocks
      (n > 4096) -> two-level flush through embed_reduce_kernel, 16 slices when the grid has at least 64 blocks (n > 32 256), the block
      count clipped to the tables the workspace holds; otherwise the LDS table is flushed with global atomics.
  gtos_segment_sum_rows: SLABS = 1 / 2 / 3 for width <= 512 / 1024 / 1536, NSRC = 1 / 2 by src2; more than 16 384 chunks -> grid-stride.
  gtos_segment_sum_stream: width / 256 = 1..6 -> <0,half> <1,-> <1,half> <2,-> <2,half> <3,->.
  gtos_segment_sum_ranges: SLABS as gtos_segment_sum_rows.

The CPU self-checks at the top emulate the kernels in fp32 torch on the stored operands, rounding where the kernels round: the honest
emulation passes every check and each of ten plausible kernel mistakes is rejected -- they prove that the GPU assertions can fail."""
import numpy as np
import pytest
import torch

from tests_support import (Guarded, GuardedFlat, _bits, assert_within, dropped_rows_bounds, drop_scale, gather_mean_bounds,
                           guarded_operand, highway_bounds, scatter_bounds, segment_sum_bounds)

gpu = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
SENT = 3.0                                     # what every output view holds before the launch (exact in bf16)
ARG_BAND, ARG_SENT = 0xA5, 0x5A                # band / sentinel bytes of the uint8 argmax output


def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    return torch.device("cuda:0")


def rnd(shape, dtype, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def hash_keep(seed, idx, p, device):
    from test_hip_parity import _hash_keep
    return _hash_keep(seed, idx.numpy(), p).to(device)


_MASKS = {}


def keep_mask(seed, rows, ld, cols, p, device):
    """the mask of a [rows, cols] block whose element (r, c) has counter r * ld + c (the last one is kept: a case asks for it again)"""
    if p <= 0:
        return torch.ones(rows, cols, dtype=torch.bool, device=device)
    key = (seed, rows, ld, cols, p, str(device))
    if key not in _MASKS:
        _MASKS.clear()
        _MASKS[key] = hash_keep(seed, torch.arange(rows).view(-1, 1) * ld + torch.arange(cols).view(1, -1), p, device)
    return _MASKS[key]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((_bits(a.contiguous()) == _bits(b.contiguous())).all())


def code(dtype):
    return 1 if dtype == BF else 0


def guard(t, on, **kw):
    return guarded_operand(t, **kw) if on else t


def refuses(rc_text, name, *args):
    from gtos_amd._lib import GtosHipError, call
    with pytest.raises(GtosHipError, match="code %s " % rc_text):
        call(name, *args)


# ================================================================================================ highway gate
def highway_operands(device, N, D, dtype, seed, guarded):
    """y = (new_x | gate), x, dout with the edges planted: new_x exactly 0.0 and -0.0 (first and last row), gate pre-activations +-30 and
    +-100 (__expf overflows), x == relu(new_x) over a whole row (dg exactly 0)."""
    assert N >= 3 and D >= 8
    y, x, dout = rnd((N, 2 * D), dtype, seed), rnd((N, D), dtype, seed + 1), rnd((N, D), dtype, seed + 2)
    for row in (0, N - 1):
        y[row, 0], y[row, 1], y[row, D - 1] = 0.0, -0.0, 0.0
    y[1, D:D + 4] = torch.tensor([30.0, -30.0, 100.0, -100.0]).to(dtype)
    y[1, 2 * D - 4:] = torch.tensor([-100.0, 100.0, -30.0, 30.0]).to(dtype)
    x[2] = y[2, :D].clamp(min=0)
    return dict(y=guard(y.to(device), guarded), x=guard(x.to(device), guarded), dout=guard(dout.to(device), guarded))


def emulate_highway(o, dtype, mutate=None):
    D = o["x"].shape[1]
    nx, g, x, go = o["y"][:, :D].float(), o["y"][:, D:].float(), o["x"].float(), o["dout"].float()
    s, r = 1.0 / (1.0 + torch.exp(-g)), nx.clamp(min=0)
    on = (nx >= 0) if mutate == ">= at the relu gate" else (nx > 0)
    got = dict(out=s * x + (1 - s) * r, dnx=torch.where(on, go * (1 - s), torch.zeros_like(go)), dg=go * (x - r) * s * (1 - s), dx=go * s)
    return {k: v.to(dtype) for k, v in got.items()}


def check_highway(tag, o, got, dtype):
    """``got``: out, dnx, dg, dx as stored.  Every element within its bound (NaN fails), dnx bitwise 0 wherever new_x <= 0 (a >= in
    place of > fails at the planted zeros), dg exactly 0 wherever x == relu(new_x)."""
    D = o["x"].shape[1]
    for name, (ref, bound) in highway_bounds(o["y"], o["x"], o["dout"], dtype).items():
        assert_within("%s %s" % (tag, name), got[name], ref, bound)
    nx = o["y"][:, :D]
    off = nx <= 0
    assert int(off.sum()) >= 3 and bool((_bits(got["dnx"].contiguous())[off] == 0).all()), tag + ": dnx is not bitwise 0 where new_x <= 0"
    flat = o["x"] == nx.clamp(min=0)
    assert int(flat.sum()) >= D and bool((got["dg"][flat] == 0).all()), tag + ": dg is not 0 where x == relu(new_x)"


# ================================================================================================ max over time + relu
def max_relu_operands(device, N, L, F, dtype, seed, guarded):
    """y [N, L, F] (handed over as [N, L * F]) and dout [N, F]: ties at positions (0, L-1) and (3, 7), an all-negative column, a column
    whose maximum is exactly 0"""
    assert N >= 4 and F >= 8
    y, dout = rnd((N, L, F), dtype, seed), rnd((N, F), dtype, seed + 1)
    y[0, 0], y[0, L - 1] = 9.0, 9.0
    if L > 7:
        y[1, 3], y[1, 7] = 9.0, 9.0
    y[2, :, 0] = -y[2, :, 0].abs() - 0.5
    y[2, :, 1] = -y[2, :, 1].abs() - 0.5
    y[2, L // 2, 1] = 0.0
    y[N - 1, :, F - 1] = -y[N - 1, :, F - 1].abs() - 0.5
    return dict(y=guard(y.reshape(N, L * F).to(device), guarded), dout=guard(dout.to(device), guarded), L=L, F=F)


def max_relu_expect(o):
    """(out, arg, dy): relu(y.max(1)[0]) in the dtype itself, the FIRST maximising position, dout there where out > 0 and 0 elsewhere"""
    L, F = o["L"], o["F"]
    y = o["y"].reshape(-1, L, F)
    m = y.max(1)[0]
    out = m.clamp(min=0)
    t = torch.arange(L, device=y.device).view(1, L, 1)
    first = torch.where(y == m[:, None], t, torch.full_like(t, L)).min(1)[0]
    hit = (t == first[:, None]) & (out[:, None] > 0)
    dy = torch.where(hit, o["dout"][:, None].expand(-1, L, -1), torch.zeros((), dtype=y.dtype, device=y.device))
    return out, first.to(torch.uint8), dy.reshape(-1, L * F)


def emulate_max_relu(o, mutate=None):
    L, F = o["L"], o["F"]
    y = o["y"].reshape(-1, L, F)
    best, at = y[:, 0].clone(), torch.zeros(y.shape[0], F, dtype=torch.long)
    for t in range(1, L):
        better = (y[:, t] >= best) if mutate == "last-max tie rule" else (y[:, t] > best)
        best, at = torch.where(better, y[:, t], best), torch.where(better, torch.full_like(at, t), at)
    out = best.clamp(min=0)
    hit = (torch.arange(L).view(1, L, 1) == at[:, None]) & (out[:, None] > 0)
    dy = torch.where(hit, o["dout"][:, None].expand(-1, L, -1), torch.zeros((), dtype=y.dtype))
    return out, at.to(torch.uint8), dy.reshape(-1, L * F)


def check_max_relu(tag, o, out, arg, dy):
    want_out, want_arg, want_dy = max_relu_expect(o)
    assert torch.equal(out, want_out), tag + ": out != relu(y.max(1)[0])"
    assert bool((out[2, :2] == 0).all()), tag + ": the planted columns give 0"
    assert torch.equal(arg, want_arg), tag + ": arg is not the first maximising position"
    assert torch.equal(dy, want_dy), tag + ": dy (every element: dout at the first maximum where out > 0, else 0)"
    print("MEASURED %s: out, arg, dy exact over %d + %d + %d elements" % (tag, out.numel(), arg.numel(), dy.numel()))


# ================================================================================================ token rows / embedding rows
def row_operands(device, N, Cc, Ct, Cp, V, dtype, seed, guarded, same_token=False):
    """feat [N, Cc] (None when Cc == 0), tok [N] over 0..V-2 (token V-1 is never used), table / the preload of dtable [V, Ct] fp32, dout
    [N, Cp] with NaN in its pad columns.  gtos_token_row_*; with Cc == 0 also gtos_embed_rows_* (Ct = dim, Cp = dim_pad)."""
    gen = torch.Generator().manual_seed(seed)
    tok = torch.randint(0, max(V - 1, 1), (N,), generator=gen)
    if same_token:
        tok[:] = min(3, V - 1)
    dout = rnd((N, Cp), dtype, seed + 3)
    dout[:, Cc + Ct:] = float("nan")
    o = dict(feat=guard(rnd((N, Cc), dtype, seed + 1).to(device), guarded) if Cc else None, tok=tok.to(device),
             table=guard(rnd((V, Ct), F32, seed + 2).to(device), guarded), dout=guard(dout.to(device), guarded),
             pre=rnd((V, Ct), F32, seed + 4).to(device) + 2.0, Cc=Cc, Ct=Ct, Cp=Cp, V=V)
    return o


def row_values(o):
    """the float64 rows before dropout: [feat | table[tok] | 0 pad]"""
    N, dv = o["tok"].shape[0], o["tok"].device
    parts = ([o["feat"].double()] if o["Cc"] else []) + [o["table"].double()[o["tok"]],
                                                          torch.zeros(N, o["Cp"] - o["Cc"] - o["Ct"], dtype=torch.float64, device=dv)]
    return torch.cat(parts, 1)


def emulate_row_fwd(o, dtype, p, seed, mutate=None):
    N, Cp = o["tok"].shape[0], o["Cp"]
    v = row_values(o).float()
    if p > 0:
        ld = o["Cc"] if mutate == "mask row stride Cc in place of Cp" else Cp
        ks = 1.0 if mutate == "missing 1/(1-p)" else 1.0 / (1.0 - torch.tensor(p, dtype=F32))
        v = torch.where(keep_mask(seed, N, ld, Cp, p, "cpu"), v * ks, torch.zeros_like(v))
    return v.to(dtype)


def check_row_fwd(tag, o, out, dtype, p, seed):
    """Every element of out [N, Cp]: p == 0 bitwise [feat | table.to(dtype) | 0]; p > 0 kept elements within stored_bound, dropped 0."""
    N, Cp = out.shape
    val = row_values(o)
    ref, bound = dropped_rows_bounds(val, keep_mask(seed, N, Cp, Cp, p, out.device), p, dtype)
    assert_within(tag + " out", out, ref, bound)
    if p == 0:
        assert same_bits(out, val.to(dtype)), tag + ": out is not bitwise [feat | table.to(dtype) | 0]"
    else:
        dropped = ~keep_mask(seed, N, Cp, Cp, p, out.device)
        assert bool((out[dropped] == 0).all()) and 0.5 * p < float(dropped.double().mean()) < 1.5 * p, tag + ": dropped elements"


def emulate_row_bwd(o, dtype, p, seed, mutate=None):
    """(dfeat, dtable) of token_row_bwd / embed_rows_bwd in fp32 torch"""
    N, Cc, Ct, Cp = o["tok"].shape[0], o["Cc"], o["Ct"], o["Cp"]
    v = o["dout"].float()
    if p > 0:
        v = torch.where(keep_mask(seed, N, Cp, Cp, p, "cpu"), v * (1.0 / (1.0 - torch.tensor(p, dtype=F32))), torch.zeros_like(v))
    dt_rows = v[:, Cc:Cc + Ct].clone()
    if mutate == "pad-column NaN let through" and Cp > Cc + Ct:
        dt_rows[:, 0] += v[:, Cc + Ct]
    base = torch.zeros_like(o["pre"]) if mutate == "dtable overwritten in place of accumulated" else o["pre"].clone()
    return (v[:, :Cc].to(dtype) if Cc else None), base.index_add(0, o["tok"], dt_rows)


def check_row_bwd(tag, o, dfeat, dtable, dtype, p, seed):
    """dfeat (None: not asked for) = masked dout[:, 0:Cc]; dtable (None: not asked for) = preload + float64 scatter of masked
    dout[:, Cc:Cc+Ct] within c_acc(count) * S, rows of unused tokens bitwise the preload, no NaN from the pad columns."""
    N, Cc, Ct, Cp = o["tok"].shape[0], o["Cc"], o["Ct"], o["Cp"]
    keep = keep_mask(seed, N, Cp, Cp, p, o["dout"].device)
    live = o["dout"][:, :Cc + Ct]
    ref, bound = dropped_rows_bounds(live.double(), keep[:, :Cc + Ct], p, dtype)
    if dfeat is not None:
        assert_within(tag + " dfeat", dfeat, ref[:, :Cc], bound[:, :Cc])
        if p == 0:
            assert same_bits(dfeat, live[:, :Cc]), tag + ": dfeat is not bitwise dout[:, 0:Cc]"
    if dtable is not None:
        tref, tbound, count = scatter_bounds(o["pre"], o["tok"], ref[:, Cc:])
        assert_within(tag + " dtable (largest count %d)" % int(count.max()), dtable, tref, tbound)
        unused = count == 0
        assert int(unused.sum()) >= 1 and same_bits(dtable[unused], o["pre"][unused]), tag + ": rows of unused tokens changed"


# ================================================================================================ relation gather-mean
def gather_operands(device, P, K, d, dtype, zero_row0, seed, guarded):
    """bank [Vb, d] (row 0 NaN when zero_row0: it must be skipped, not multiplied by 0), idx [P, K]: row 0 all zero, row i with
    (i - 1) % K + 1 live entries in front, zeros behind; in the second half the zeros come first"""
    Vb = 41
    bank = rnd((Vb, d), dtype, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    if zero_row0:
        bank[0] = float("nan")
        idx = torch.randint(1, Vb, (P, K), generator=gen)
        live = (torch.arange(P).view(-1, 1) - 1) % K + 1
        idx[torch.arange(K).view(1, -1) >= live] = 0
        idx[P // 2:] = idx[P // 2:].flip(1)
        idx[0] = 0
    else:
        idx = torch.randint(0, Vb, (P, K), generator=gen)
        idx[0] = 0
    return dict(bank=guard(bank.to(device), guarded), idx=idx.to(device), K=K)


def emulate_gather_mean(o, dtype, zero_row0, mutate=None):
    bank, idx = o["bank"].float(), o["idx"]
    acc, cnt = torch.zeros(idx.shape[0], bank.shape[1]), torch.zeros(idx.shape[0], 1)
    for k in range(idx.shape[1]):
        live = ((idx[:, k] != 0) | (not zero_row0)).float()[:, None]
        acc, cnt = acc + torch.nan_to_num(bank[idx[:, k]]) * live, cnt + live
    if zero_row0:
        acc = acc * (1.0 / (torch.full_like(cnt, idx.shape[1]) if mutate == "mean over K in place of the live count" else cnt.clamp(min=1)))
    return acc.to(dtype)


def check_gather_mean(tag, o, out, dtype, zero_row0):
    if zero_row0:
        assert_within(tag + " out", out, *gather_mean_bounds(o["bank"], o["idx"], dtype))
        assert bool((out[0] == 0).all()), tag + ": an all-zero index row gives zeros"
    else:
        assert o["K"] == 1 and same_bits(out, o["bank"][o["idx"][:, 0]]), tag + ": K = 1 without the row-0 rule is a bitwise copy"
        print("MEASURED %s: bitwise copy of %d elements" % (tag, out.numel()))


# ================================================================================================ packed paths
def packed_case(device, L, R, max_len, V, seed):
    """bank [L, R] of labels 1..V-1 (0 behind each path's end), the PackPlan of its lengths, offs padded to L + 1 entries (the steps past
    ``max_len`` are empty) and the token of every packed row from a plain loop over (step, sorted path)."""
    from gtos_amd.gru import PackPlan
    gen = torch.Generator().manual_seed(seed)
    length = torch.randint(1, max_len + 1, (R,), generator=gen)
    length[R // 2] = max_len
    bank = torch.randint(1, V, (L, R), generator=gen)
    for r in range(R):
        bank[int(length[r]):, r] = 0
    plan = PackPlan.of_lengths(length.to(device), L)
    order = plan.order32.cpu().tolist()
    want = []
    for t, a in enumerate(plan.batch_sizes):
        for m in range(a):
            want.append(int(bank[t, order[m]]))
    assert len(want) == plan.N == int(length.sum()) and plan.L == max_len
    offs = torch.tensor(plan.offs + [plan.N] * (L - plan.L), dtype=torch.int32)
    return bank.to(device), plan, offs.to(device), torch.tensor(want, dtype=torch.int64, device=device)


def emulate_onehot(tokens, vp, dim_pad, mutate=None):
    oh = torch.nn.functional.one_hot(tokens, vp).to(BF)
    if mutate == "one-hot loop stops after one trip":
        oh[:, min(vp, dim_pad):] = SENT
    return oh


def check_onehot(tag, onehot, tokens, vp):
    assert torch.equal(onehot, torch.nn.functional.one_hot(tokens, vp).to(BF)), tag + ": onehot"


# ================================================================================================ segmented sums
def make_csr(counts, chunk=64, empty_chunk_in=None):
    """A CSR chunk list as the trie builds it: node u owns counts[u] consecutive entries of the row list, cut into chunks of at most
    ``chunk``; a node of several chunks is heavy (slot >= 0).  ``empty_chunk_in``: that (heavy) node gets one more chunk without rows
    behind its first."""
    cn, cs, cc, sl, heavy_node, pos = [], [], [], [], [], 0
    for u, n in enumerate(counts):
        sizes = [min(chunk, n - k) for k in range(0, n, chunk)] or [0]
        if u == empty_chunk_in:
            assert len(sizes) > 1
            sizes.insert(1, 0)
        slot = -1
        if len(sizes) > 1:
            slot = len(heavy_node)
            heavy_node.append(u)
        at = pos
        for s in sizes:
            cn.append(u); cs.append(at); cc.append(s); sl.append(slot)
            at += s
        pos += n
    return dict(chunk_node=np.asarray(cn, np.int32), chunk_start=np.asarray(cs, np.int32), chunk_cnt=np.asarray(cc, np.int32),
                chunk_slot=np.asarray(sl, np.int32), heavy_node=np.asarray(heavy_node, np.int32), total=pos, n_nodes=len(counts),
                node_of_pos=np.repeat(np.arange(len(counts)), counts))


SEG_COUNTS = [0, 1, 2, 3, 5, 63, 64, 130, 0, 700, 1, 0, 2, 64, 65, 3, 0]       # chunk sizes 0 1 2 3 5 63 64; heavy: 130, 700, 65


def emulate_segment_sum(csr, rows, src, mutate=None):
    """seg_sum_kernel + seg_finish_kernel in fp32 torch: per chunk an fp32 sum, chunks of a node added up, one rounding to bf16"""
    out = torch.zeros(csr["n_nodes"], src.shape[1])
    for node, start, cnt in zip(csr["chunk_node"], csr["chunk_start"], csr["chunk_cnt"]):
        ids = rows[start:start + cnt]
        if mutate == "a chunk's last row dropped" and cnt > 1:
            ids = ids[:-1]
        if mutate == "a row counted twice when cnt % UN != 0" and cnt % 4:
            ids = torch.cat([ids, ids[-1:]])
        out[node] += src[ids.long()].float().sum(0)
    return out.to(BF)


def check_segment_sum(tag, csr, rows, src, dst):
    """dst [n_nodes, W] bf16 against the float64 sums of the stored rows: every node held to ITS c_acc(cnt) * S, empty nodes exactly 0"""
    node = torch.as_tensor(csr["node_of_pos"], device=src.device).long()
    ref, bound = segment_sum_bounds(src.double()[rows.long()], node, csr["n_nodes"])
    assert_within(tag, dst, ref, bound)
    empty = torch.bincount(node, minlength=csr["n_nodes"]) == 0
    assert bool((dst[empty] == 0).all()), tag + ": empty nodes are exactly 0"


# ================================================================================================ CPU self-checks
MUTATIONS = [">= at the relu gate", "last-max tie rule", "missing 1/(1-p)", "mask row stride Cc in place of Cp", "a chunk's last row dropped",
             "a row counted twice when cnt % UN != 0", "mean over K in place of the live count", "one-hot loop stops after one trip",
             "dtable overwritten in place of accumulated", "pad-column NaN let through"]


def cpu_checks(mutate=None):
    """Every check of this file on the CPU emulation of its kernel (bf16, small shapes); ``mutate`` plants one mistake."""
    o = highway_operands("cpu", 37, 40, BF, 1, False)
    check_highway("emulated highway", o, emulate_highway(o, BF, mutate), BF)
    o = max_relu_operands("cpu", 9, 12, 24, BF, 2, False)
    check_max_relu("emulated max_relu", o, *emulate_max_relu(o, mutate))
    o = row_operands("cpu", 50, 16, 30, 48, 23, BF, 3, False)
    for p in (0.0, 0.25):
        check_row_fwd("emulated token_row_fwd p=%g" % p, o, emulate_row_fwd(o, BF, p, 77, mutate), BF, p, 77)
        check_row_bwd("emulated token_row_bwd p=%g" % p, o, *emulate_row_bwd(o, BF, p, 77, mutate), BF, p, 77)
    o = gather_operands("cpu", 29, 4, 16, BF, 1, 4, False)
    check_gather_mean("emulated gather_mean", o, emulate_gather_mean(o, BF, 1, mutate), BF, 1)
    o = gather_operands("cpu", 29, 1, 16, BF, 0, 5, False)
    check_gather_mean("emulated gather_mean copy", o, emulate_gather_mean(o, BF, 0, mutate), BF, 0)
    tokens = torch.randint(0, 150, (40,), generator=torch.Generator().manual_seed(6))
    check_onehot("emulated onehot", emulate_onehot(tokens, 160, 32, mutate), tokens, 160)
    csr = make_csr(SEG_COUNTS, empty_chunk_in=7)
    rows = torch.randperm(csr["total"] + 37, generator=torch.Generator().manual_seed(7))[:csr["total"]].to(torch.int32)
    src = rnd((csr["total"] + 37, 16), BF, 8)
    check_segment_sum("emulated segment sum", csr, rows, src, emulate_segment_sum(csr, rows, src, mutate))


def test_checks_accept_the_honest_emulations():
    cpu_checks()


@pytest.mark.parametrize("mutate", MUTATIONS)
def test_checks_reject(mutate):
    with pytest.raises(AssertionError) as e:
        cpu_checks(mutate)
    print("REJECTED %s: %s" % (mutate, str(e.value).splitlines()[0][:200]))


# ================================================================================================ GPU: highway gate
def t32(a, device):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(device)


def untouched(*views):
    return all(bool((v == SENT).all()) for v in views)


def run_highway(tag, N, D, dtype, seed):
    from gtos_amd._lib import call, ptr, stream
    d = dev()
    o = highway_operands(d, N, D, dtype, seed, True)
    out, dy, dx = (Guarded(N, w, dtype, d, init=SENT) for w in (D, 2 * D, D))
    call("gtos_highway_fwd", code(dtype), N, D, ptr(o["y"]), ptr(o["x"]), ptr(out.view), stream())
    out.check(tag + " out")
    call("gtos_highway_bwd", code(dtype), N, D, ptr(o["y"]), ptr(o["x"]), ptr(o["dout"]), ptr(dy.view), ptr(dx.view), stream())
    for g_, w in ((out, "out"), (dy, "dy"), (dx, "dx")):
        g_.check("%s %s" % (tag, w))
    check_highway(tag, o, dict(out=out.view, dnx=dy.view[:, :D], dg=dy.view[:, D:], dx=dx.view), dtype)


@gpu
@DTYPES
@pytest.mark.parametrize("N,D", [(3, 8), (77, 40), (301, 1024)])
def test_highway_guarded(N, D, dtype):
    """highway_fwd_kernel / highway_bwd_kernel, first lap: one chunk per row (D = 8, three rows: one partial block), D = 40 (5 chunks: the
    row / chunk split is no power of two), D = 1024 over 151 blocks; the planted zeros, saturated gates and x == relu(new_x) in each."""
    run_highway("highway %s N=%d D=%d" % (str(dtype)[6:], N, D), N, D, dtype, N + D)


@gpu
def test_highway_second_lap_guarded():
    """N = 16 400, D = 1024, bf16: 2 099 200 work items over the 8192 x 256 grid -- items 2 097 152.. (rows 16 384..) are a second lap;
    the planted edges of the last row are among them."""
    run_highway("highway second lap", 16400, 1024, BF, 5)


@gpu
@pytest.mark.parametrize("D", [0, 12])
def test_highway_refuses_bad_widths(D):
    from gtos_amd._lib import ptr, stream
    d = dev()
    o = highway_operands(d, 5, 16, BF, 1, True)
    out, dy, dx = (Guarded(5, w, BF, d, init=SENT) for w in (16, 32, 16))
    refuses("-24", "gtos_highway_fwd", 1, 5, D, ptr(o["y"]), ptr(o["x"]), ptr(out.view), stream())
    refuses("-24", "gtos_highway_bwd", 1, 5, D, ptr(o["y"]), ptr(o["x"]), ptr(o["dout"]), ptr(dy.view), ptr(dx.view), stream())
    for g_ in (out, dy, dx):
        g_.check("refused highway")
    assert untouched(out.view, dy.view, dx.view)


# ================================================================================================ GPU: max over time + relu
def max_relu_buffers(d, N, L, F, dtype):
    out = Guarded(N, F, dtype, d, init=SENT)
    arg = Guarded(N, F, torch.uint8, d, init=ARG_SENT, band=ARG_BAND)
    dy = Guarded(N, max(L, 1) * F, dtype, d, init=SENT)
    return out, arg, dy


def run_max_relu(tag, N, L, F, dtype, seed):
    from gtos_amd._lib import call, ptr, stream
    d = dev()
    o = max_relu_operands(d, N, L, F, dtype, seed, True)
    out, arg, dy = max_relu_buffers(d, N, L, F, dtype)
    call("gtos_max_relu_fwd", code(dtype), N, L, F, ptr(o["y"]), ptr(out.view), ptr(arg.view), stream())
    out.check(tag + " out")
    arg.check(tag + " arg")
    # backward from the forward's own stored out and arg (they sit in NaN / band bytes already)
    call("gtos_max_relu_bwd", code(dtype), N, L, F, ptr(out.view), ptr(arg.view), ptr(o["dout"]), ptr(dy.view), stream())
    for g_, w in ((out, "out"), (arg, "arg"), (dy, "dy")):
        g_.check("%s %s" % (tag, w))
    check_max_relu(tag, o, out.view, arg.view, dy.view)


@gpu
@DTYPES
@pytest.mark.parametrize("N,L,F", [(5, 1, 8), (33, 12, 24), (300, 12, 8), (9, 255, 24)])
def test_max_relu_guarded(N, L, F, dtype):
    """max_relu_fwd_kernel / max_relu_bwd_kernel: L = 1 (no loop trip) and L = 255 (the largest position a byte of arg holds), F = 8 (one
    chunk per sample) and F = 24, one and two blocks; ties at (0, L-1) and (3, 7), an all-negative column, a column with maximum 0."""
    run_max_relu("max_relu %s N=%d L=%d F=%d" % (str(dtype)[6:], N, L, F), N, L, F, dtype, N + L + F)


@gpu
def test_max_relu_second_lap_guarded():
    """N = 262 200, L = 2, F = 64, bf16: 2 097 600 work items, the last 448 of them (samples 262 144..) on the second lap"""
    run_max_relu("max_relu second lap", 262200, 2, 64, BF, 6)


@gpu
@pytest.mark.parametrize("L,F", [(0, 8), (256, 8), (12, 12)])
def test_max_relu_refuses_bad_shapes(L, F):
    """L = 0, L = 256 (a position would not fit a byte) and F % 8 != 0 return -24 and write nothing"""
    from gtos_amd._lib import ptr, stream
    d = dev()
    o = max_relu_operands(d, 4, 256, 16, BF, 1, True)
    out, arg, dy = max_relu_buffers(d, 4, 256, 16, BF)
    refuses("-24", "gtos_max_relu_fwd", 1, 4, L, F, ptr(o["y"]), ptr(out.view), ptr(arg.view), stream())
    refuses("-24", "gtos_max_relu_bwd", 1, 4, L, F, ptr(out.view), ptr(arg.view), ptr(o["dout"]), ptr(dy.view), stream())
    for g_ in (out, arg, dy):
        g_.check("refused max_relu")
    assert untouched(out.view, dy.view) and bool((arg.view == ARG_SENT).all())


# ================================================================================================ GPU: token rows
def run_token_row(tag, N, Cc, Ct, V, dtype, p, seed, same_token=False, outputs=("dfeat", "dtable")):
    from gtos_amd._lib import call, ptr, stream
    d = dev()
    Cp = (Cc + Ct + 7) // 8 * 8
    o = row_operands(d, N, Cc, Ct, Cp, V, dtype, seed, True, same_token)
    sd = 4242 + seed
    out = Guarded(N, Cp, dtype, d, init=SENT)
    call("gtos_token_row_fwd", code(dtype), N, Cc, Ct, Cp, ptr(o["feat"]), ptr(o["tok"]), ptr(o["table"]), ptr(out.view), p,
         sd if p > 0 else 0, stream())
    out.check(tag + " out")
    check_row_fwd(tag, o, out.view, dtype, p, sd)
    dfeat = Guarded(N, Cc, dtype, d, init=SENT) if Cc and "dfeat" in outputs else None
    dtab = Guarded(V, Ct, F32, d, init=o["pre"]) if "dtable" in outputs else None
    call("gtos_token_row_bwd", code(dtype), N, Cc, Ct, Cp, ptr(o["dout"]), ptr(o["tok"]), None if dfeat is None else ptr(dfeat.view),
         None if dtab is None else ptr(dtab.view), p, sd if p > 0 else 0, stream())
    for g_, w in ((dfeat, "dfeat"), (dtab, "dtable")):
        if g_ is not None:
            g_.check("%s %s" % (tag, w))
    check_row_bwd(tag, o, None if dfeat is None else dfeat.view, None if dtab is None else dtab.view, dtype, p, sd)


@gpu
@DTYPES
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("N,Cc,Ct", [(50, 16, 30), (300, 8, 8), (37, 0, 1), (129, 16, 1)])
def test_token_row_guarded(N, Cc, Ct, p, dtype):
    """token_row_fwd_kernel / token_row_bwd_kernel at pads of 2, 0, 7 and 7 columns; (0, 1): no feature columns, feat = NULL.  p = 0:
    bitwise [feat | table.to(dtype) | 0]; p = 0.25: every element follows the mask at counter row * Cp + column.  Backward: dfeat the
    masked dout, dtable accumulated onto a non-zero preload, the unused token's row bitwise unchanged, NaN in dout's pad columns."""
    run_token_row("token_row %s N=%d Cc=%d Ct=%d p=%g" % (str(dtype)[6:], N, Cc, Ct, p), N, Cc, Ct, 23, dtype, p, N + Cc + Ct)


@gpu
@DTYPES
@pytest.mark.parametrize("outputs,same_token", [(("dtable",), False), (("dfeat",), False), (("dfeat", "dtable"), True)])
def test_token_row_backward_optional_outputs_and_one_token(outputs, same_token, dtype):
    """dfeat = NULL and dtable = NULL one at a time (the other output stays correct); every row carrying the same token (300 atomics
    per table word)"""
    tag = "token_row %s outputs=%s same_token=%d" % (str(dtype)[6:], "+".join(outputs), same_token)
    run_token_row(tag, 300, 16, 30, 23, dtype, 0.25, 11, same_token, outputs)


@gpu
def test_token_row_second_lap_guarded():
    """N = 1 048 700, Cc = Ct = 8 (Cp = 16), bf16, p = 0.25: 2 097 400 work items, rows 1 048 576.. on the second lap, forward and
    backward; the table gradient adds about a thousand rows per token"""
    run_token_row("token_row second lap", 1048700, 8, 8, 1001, BF, 0.25, 7)


@gpu
@pytest.mark.parametrize("Cc,Ct,Cp", [(12, 30, 48), (16, 0, 16), (16, 30, 56), (16, 30, 40)])
def test_token_row_refuses_bad_shapes(Cc, Ct, Cp):
    from gtos_amd._lib import ptr, stream
    d = dev()
    o = row_operands(d, 9, 16, 30, 48, 23, BF, 1, True)
    out, dfeat, dtab = Guarded(9, 56, BF, d, init=SENT), Guarded(9, 16, BF, d, init=SENT), Guarded(23, 30, F32, d, init=SENT)
    refuses("-24", "gtos_token_row_fwd", 1, 9, Cc, Ct, Cp, ptr(o["feat"]), ptr(o["tok"]), ptr(o["table"]), ptr(out.view), 0.0, 0, stream())
    refuses("-24", "gtos_token_row_bwd", 1, 9, Cc, Ct, Cp, ptr(o["dout"]), ptr(o["tok"]), ptr(dfeat.view), ptr(dtab.view), 0.0, 0, stream())
    for g_ in (out, dfeat, dtab):
        g_.check("refused token_row")
    assert untouched(out.view, dfeat.view, dtab.view)


# ================================================================================================ GPU: relation gather-mean
def run_gather_mean(tag, P, K, dd, dtype, zero_row0, seed):
    from gtos_amd._lib import call, ptr, stream
    d = dev()
    o = gather_operands(d, P, K, dd, dtype, zero_row0, seed, True)
    out = Guarded(P, dd, dtype, d, init=SENT)
    call("gtos_relation_gather_mean", code(dtype), P, K, dd, ptr(o["bank"]), ptr(o["idx"]), zero_row0, ptr(out.view), stream())
    out.check(tag)
    check_gather_mean(tag, o, out.view, dtype, zero_row0)


@gpu
@DTYPES
@pytest.mark.parametrize("P,K,dd,zero_row0", [(37, 1, 8, 1), (37, 4, 8, 1), (300, 1, 64, 1), (300, 4, 64, 1), (37, 1, 8, 0), (300, 1, 64, 0)])
def test_gather_mean_guarded(P, K, dd, zero_row0, dtype):
    """gather_mean_kernel: the evaluation lookup (zero_row0 = 1: rows with 0..K live entries, zeros in front of and behind them, bank row
    0 holding NaN) and the training lookup (K = 1, zero_row0 = 0: a bitwise copy, row 0 included)"""
    run_gather_mean("gather_mean %s P=%d K=%d d=%d zero_row0=%d" % (str(dtype)[6:], P, K, dd, zero_row0), P, K, dd, dtype, zero_row0, P + K + dd)


@gpu
def test_gather_mean_second_lap_guarded():
    """P = 262 200, d = 64, K = 2, bf16: 2 097 600 work items, rows 262 144.. on the second lap"""
    run_gather_mean("gather_mean second lap", 262200, 2, 64, BF, 1, 9)


@gpu
def test_gather_mean_refuses_bad_width():
    from gtos_amd._lib import ptr, stream
    d = dev()
    o = gather_operands(d, 9, 2, 16, BF, 1, 1, True)
    out = Guarded(9, 16, BF, d, init=SENT)
    refuses("-23", "gtos_relation_gather_mean", 1, 9, 2, 12, ptr(o["bank"]), ptr(o["idx"]), 1, ptr(out.view), stream())
    out.check("refused gather_mean")
    assert untouched(out.view)


# ================================================================================================ GPU: embedding rows, forward
EMBED_DIMS = [(100, 104), (100, 128), (8, 8), (1, 8)]


@gpu
@DTYPES
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("dim,dim_pad", EMBED_DIMS)
def test_embed_rows_fwd_guarded(dim, dim_pad, p, dtype):
    """embed_rows_fwd_kernel against its own restatement (not against the packed-path kernel): pads of 4, 28, 0 and 7 columns; p = 0
    bitwise table[tok].to(dtype) with zero pad columns, p = 0.3 every element by the mask at counter row * dim_pad + column"""
    from gtos_amd._lib import call, ptr, stream
    d, n, V = dev(), 301, 23
    tag = "embed_rows_fwd %s dim=%d/%d p=%g" % (str(dtype)[6:], dim, dim_pad, p)
    o = row_operands(d, n, 0, dim, dim_pad, V, dtype, dim + dim_pad, True)
    out = Guarded(n, dim_pad, dtype, d, init=SENT)
    sd = 99 + dim
    call("gtos_embed_rows_fwd", code(dtype), n, dim, dim_pad, ptr(o["tok"]), ptr(o["table"]), ptr(out.view), p, sd if p > 0 else 0, stream())
    out.check(tag)
    check_row_fwd(tag, o, out.view, dtype, p, sd)


def run_packed_paths(tag, L, R, max_len, dim, dim_pad, vp, dtype, p, seed, with_onehot=True, with_tokens=True):
    from gtos_amd._lib import call, ptr, stream
    d = dev()
    V = vp - 3
    bank, plan, offs, want = packed_case(d, L, R, max_len, V, seed)
    N = plan.N
    o = dict(feat=None, tok=want, table=guarded_operand(rnd((V, dim), F32, seed + 1).to(d)), Cc=0, Ct=dim, Cp=dim_pad)
    x = Guarded(N, dim_pad, dtype, d, init=SENT)
    onehot = Guarded(N, vp, BF, d, init=SENT)
    tokens = GuardedFlat(N, torch.int64, d, init=-7, band=0x5A5A5A5A5A5A5A5A)
    sd = 31 + seed
    call("gtos_embed_packed_paths", code(dtype), L, R, N, ptr(bank), ptr(plan.order32), ptr(offs), ptr(o["table"]), dim, dim_pad, ptr(x.view),
         p, sd if p > 0 else 0, ptr(onehot.view) if with_onehot else None, vp, ptr(tokens.view) if with_tokens else None, stream())
    for g_, w in ((x, "x"), (onehot, "onehot"), (tokens, "tokens")):
        g_.check("%s %s" % (tag, w))
    check_row_fwd(tag, o, x.view, dtype, p, sd)
    if with_onehot:
        check_onehot(tag, onehot.view, want, vp)
    else:
        assert untouched(onehot.view), tag + ": onehot = NULL yet the buffer changed"
    if with_tokens:
        assert torch.equal(tokens.view, want), tag + ": tokens"
    else:
        assert bool((tokens.view == -7).all())
    print("MEASURED %s: tokens and onehot exact over %d rows" % (tag, N))


@gpu
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("L,R,max_len,dim,dim_pad,vp,dtype", [
    (1, 300, 1, 100, 128, 88, BF), (7, 300, 5, 100, 128, 88, BF), (64, 60, 61, 100, 128, 88, BF), (64, 60, 64, 30, 32, 160, BF),
    (7, 300, 7, 30, 32, 160, F32), (7, 300, 5, 100, 104, 88, F32), (7, 50, 5, 8, 8, 88, BF), (7, 50, 7, 1, 8, 160, BF)],
    ids=lambda v: str(v).replace("torch.", ""))
def test_embed_packed_paths_guarded(L, R, max_len, dim, dim_pad, vp, dtype, p):
    """embed_packed_paths_kernel against the sort order and step offsets of PackPlan and a plain loop over (step, sorted path): L = 1, 7
    and 64 (all 65 offsets of the kernel's LDS copy), steps past the longest path left empty (equal trailing offsets), vp = 88 beside
    dim_pad = 128 (fewer one-hot chunks than threads per row) and vp = 160 beside dim_pad = 32 or 8 (5 / 20 trips of the one-hot loop),
    x in bf16 and fp32."""
    tag = "packed_paths %s L=%d R=%d max_len=%d dim=%d/%d vp=%d p=%g" % (str(dtype)[6:], L, R, max_len, dim, dim_pad, vp, p)
    run_packed_paths(tag, L, R, max_len, dim, dim_pad, vp, dtype, p, L + R + dim)


@gpu
@pytest.mark.parametrize("with_onehot,with_tokens", [(False, True), (True, False)])
def test_embed_packed_paths_optional_outputs(with_onehot, with_tokens):
    """onehot = NULL / tokens = NULL: the other outputs stay correct and the absent one's buffer is not written"""
    run_packed_paths("packed_paths onehot=%d tokens=%d" % (with_onehot, with_tokens), 7, 300, 6, 30, 32, 160, BF, 0.3, 3, with_onehot, with_tokens)


@gpu
def test_embed_packed_paths_refuses_65_steps():
    """L = 65: the offsets would not fit the kernel's LDS copy -- -24 and nothing written"""
    from gtos_amd._lib import ptr, stream
    d = dev()
    bank, plan, offs, want = packed_case(d, 65, 20, 65, 85, 1)
    table = rnd((85, 30), F32, 2).to(d)
    x, onehot = Guarded(plan.N, 32, BF, d, init=SENT), Guarded(plan.N, 88, BF, d, init=SENT)
    refuses("-24", "gtos_embed_packed_paths", 1, 65, 20, plan.N, ptr(bank), ptr(plan.order32), ptr(offs), ptr(table), 30, 32, ptr(x.view), 0.0, 0,
            ptr(onehot.view), 88, None, stream())
    x.check("refused packed_paths x")
    onehot.check("refused packed_paths onehot")
    assert untouched(x.view, onehot.view)


# ================================================================================================ GPU: embedding rows, backward
def embed_bwd_grid(n, V, dim_pad, ws_tables):
    """(blocks of embed_rows_bwd_kernel, tables of the workspace it writes) by the rule stated in the entry point's comments"""
    lds = V * dim_pad * 4 <= 60 * 1024
    nb = min(2048, max(1, (n + 511) // 512))
    two_level = lds and ws_tables and nb > 8
    if two_level:
        nb = min(nb, ws_tables)
    rpb = (n + nb - 1) // nb
    grid = (n + rpb - 1) // rpb
    return grid, (grid if two_level else 0)


def run_embed_bwd(tag, n, V, dim, dim_pad, dtype, p, seed, ws_tables=0, same_token=False, want_grid=None):
    from gtos_amd._lib import call, ptr, stream
    d = dev()
    o = row_operands(d, n, 0, dim, dim_pad, V, dtype, seed, True, same_token)
    dtab = Guarded(V, dim, F32, d, init=o["pre"])
    words = V * dim_pad
    ws = GuardedFlat(ws_tables * words, F32, d, init=SENT) if ws_tables else None
    sd = 555 + seed
    grid, written = embed_bwd_grid(n, V, dim_pad, ws_tables)
    assert want_grid is None or (grid, written) == want_grid, (tag, grid, written)
    call("gtos_embed_rows_bwd", code(dtype), n, V, dim, dim_pad, ptr(o["tok"]), ptr(o["dout"]), ptr(dtab.view), p, sd if p > 0 else 0,
         None if ws is None else ptr(ws.view), ws_tables * words * 4, stream())
    dtab.check(tag + " dtable")
    if ws is not None:
        ws.check(tag + " workspace")
        assert untouched(ws.view[written * words:]), tag + ": the workspace behind the grid's %d tables changed" % written
    check_row_bwd(tag, o, None, dtab.view, dtype, p, sd)


# (n, V, dim, dim_pad, workspace tables, (blocks, workspace tables written)): the route each case takes
EMBED_BWD_ROUTES = {
    "lds-direct-small": (50, 23, 30, 32, 0, (1, 0)),
    "lds-direct-no-workspace": (5000, 23, 30, 32, 0, (10, 0)),
    "lds-direct-few-blocks-workspace-unused": (4000, 23, 30, 32, 10, (8, 0)),
    "two-level-1-slice": (5000, 23, 30, 32, 10, (10, 10)),
    "two-level-1-slice-roomy-workspace": (5000, 23, 30, 32, 12, (10, 10)),
    "two-level-16-slices": (33000, 90, 100, 104, 65, (65, 65)),
    "two-level-clipped-to-9-tables": (33000, 90, 100, 104, 9, (9, 9)),
    "global-atomics": (5000, 481, 30, 32, 10, (10, 0)),
    "lds-boundary-60KiB": (5000, 480, 30, 32, 10, (10, 10)),
}


@gpu
@DTYPES
@pytest.mark.parametrize("route", list(EMBED_BWD_ROUTES))
def test_embed_rows_bwd_routes_guarded(route, dtype):
    """embed_rows_bwd_kernel<T, lds> and embed_reduce_kernel, every route at its smallest shape: dtable = non-zero preload + float64
    scatter within c_acc(count) * S, NaN in dout's pad columns, the unused token's row bitwise unchanged, the workspace in guard bands
    and unwritten behind the grid's tables (not at all on the direct and the global-atomics routes)."""
    n, V, dim, dim_pad, ws_tables, want = EMBED_BWD_ROUTES[route]
    run_embed_bwd("embed_rows_bwd %s %s" % (str(dtype)[6:], route), n, V, dim, dim_pad, dtype, 0.0, n + V, ws_tables, want_grid=want)


@gpu
@DTYPES
@pytest.mark.parametrize("n,ws_tables,same_token,p", [(5000, 10, True, 0.0), (5000, 0, True, 0.0), (5000, 10, False, 0.3), (50, 0, False, 0.3),
                                                      (33000, 65, False, 0.3)])
def test_embed_rows_bwd_one_token_and_dropout(n, ws_tables, same_token, p, dtype):
    """every row carrying the same token (5000 terms per word, on the two-level and the direct route); p = 0.3 with the mask at
    counter row * dim_pad + column"""
    V, dim, dim_pad = (90, 100, 104) if n > 30000 else (23, 30, 32)
    tag = "embed_rows_bwd %s n=%d ws=%d same_token=%d p=%g" % (str(dtype)[6:], n, ws_tables, same_token, p)
    run_embed_bwd(tag, n, V, dim, dim_pad, dtype, p, n + ws_tables + 1, ws_tables, same_token)


@gpu
def test_embed_rows_bwd_refuses_a_workspace_below_one_table():
    from gtos_amd._lib import ptr, stream
    d = dev()
    n, V, dim, dim_pad = 5000, 23, 30, 32
    o = row_operands(d, n, 0, dim, dim_pad, V, BF, 1, True)
    dtab = Guarded(V, dim, F32, d, init=o["pre"])
    ws = GuardedFlat(V * dim_pad - 1, F32, d, init=SENT)
    refuses("-24", "gtos_embed_rows_bwd", 1, n, V, dim, dim_pad, ptr(o["tok"]), ptr(o["dout"]), ptr(dtab.view), 0.0, 0, ptr(ws.view),
            (V * dim_pad - 1) * 4, stream())
    refuses("-24", "gtos_embed_rows_bwd", 1, n, V, dim, 28, ptr(o["tok"]), ptr(o["dout"]), ptr(dtab.view), 0.0, 0, None, 0, stream())
    dtab.check("refused embed_rows_bwd dtable")
    ws.check("refused embed_rows_bwd workspace")
    assert same_bits(dtab.view, o["pre"]) and untouched(ws.view)


# ================================================================================================ GPU: segmented sums
def seg_case(d, csr, W, n_sources, use_rows, seed, ld_gap=8):
    """Device copies of a CSR, guarded sources (NaN in the leading-dimension gap and around) and guarded destinations / heavy slots"""
    total, n_nodes, nh = csr["total"], csr["n_nodes"], len(csr["heavy_node"])
    n_src = total + 37 if use_rows else max(total, 1)
    rows = np.random.RandomState(seed).permutation(n_src)[:total] if use_rows else np.arange(total)
    c = dict(rows=t32(rows, d), cn=t32(csr["chunk_node"], d), cs=t32(csr["chunk_start"], d), cc=t32(csr["chunk_cnt"], d),
             sl=t32(csr["chunk_slot"], d), hn=t32(csr["heavy_node"], d), nh=nh, ld=W + ld_gap, use_rows=use_rows)
    c["src"] = [guarded_operand(rnd((n_src, W), BF, seed + 1 + q).to(d), ld=W + ld_gap) for q in range(n_sources)]
    c["dst"] = [Guarded(n_nodes, W, BF, d, ld=W + ld_gap, init=SENT) for _ in range(n_sources)]
    c["heavy"] = [Guarded(max(nh, 1), W, F32, d, init=0.0) for _ in range(n_sources)]
    return c


def seg_finish_and_check(tag, csr, c, W):
    from gtos_amd._lib import call, ptr, stream
    for q, (src, dst, heavy) in enumerate(zip(c["src"], c["dst"], c["heavy"])):
        heavy.check("%s heavy %d" % (tag, q))
        dst.check("%s dst %d before finish" % (tag, q))
        if c["nh"]:
            assert untouched(dst.view[c["hn"].long()]), tag + ": a heavy node's row was written before seg_finish_kernel"
            call("gtos_segment_sum_finish", c["nh"], ptr(c["hn"]), ptr(heavy.view), W, ptr(dst.view), c["ld"], stream())
        dst.check("%s dst %d" % (tag, q))
        check_segment_sum("%s source %d" % (tag, q), csr, c["rows"], src, dst.view)


def run_seg_rows(tag, W, n_sources, use_rows, counts, seed, empty_chunk_in=None, ld_gap=8):
    from gtos_amd._lib import call, ptr, stream
    d = dev()
    csr = make_csr(counts, empty_chunk_in=empty_chunk_in)
    c = seg_case(d, csr, W, n_sources, use_rows, seed, ld_gap)
    two = n_sources == 2
    call("gtos_segment_sum_rows", len(csr["chunk_node"]), ptr(c["rows"]) if use_rows else None, ptr(c["cn"]), ptr(c["cs"]), ptr(c["cc"]),
         ptr(c["sl"]), ptr(c["src"][0]), ptr(c["src"][1]) if two else None, c["ld"], W, ptr(c["dst"][0].view),
         ptr(c["dst"][1].view) if two else None, c["ld"], ptr(c["heavy"][0].view), ptr(c["heavy"][1].view) if two else None, stream())
    seg_finish_and_check(tag, csr, c, W)


@gpu
@pytest.mark.parametrize("n_sources", [1, 2])
@pytest.mark.parametrize("W,use_rows", [(8, True), (512, False), (520, True), (1024, True), (1528, False), (1528, True)])
def test_segment_sum_rows_guarded(W, use_rows, n_sources):
    """seg_sum_kernel<SLABS, NSRC> + seg_finish_kernel: widths 8 (one lane), 512 (a full slab), 520 and 1528 (a partial last slab of
    SLABS = 2 and 3), 1024; one and two sources; a row list and rows = NULL (consecutive rows); chunk sizes 0 1 2 3 5 63 64, heavy nodes of
    2, 3 and 11 chunks, one of them with a chunk without rows; ld_src = ld_dst = W + 8 with NaN in the gap."""
    tag = "segment_sum_rows W=%d sources=%d rows=%s" % (W, n_sources, "list" if use_rows else "NULL")
    run_seg_rows(tag, W, n_sources, use_rows, SEG_COUNTS, W + n_sources, empty_chunk_in=7)


@gpu
def test_segment_sum_rows_grid_stride_guarded():
    """16 500 chunks at width 8: 4096 blocks of four waves, the last 116 chunks on a second lap (the three-stage prefetch of chunk
    records and row ids across the lap)"""
    counts = np.random.RandomState(3).choice([0, 1, 2, 3, 5], size=16500).tolist()
    run_seg_rows("segment_sum_rows grid stride", 8, 1, True, counts, 3)


def wave_offsets(csr, rows_per_wave):
    """Chunk indices cutting the list into waves of about ``rows_per_wave`` rows, plus: a wave that STARTS with an empty node, a wave
    that ENDS with one, and an empty wave (two equal offsets)."""
    cs, n_chunks = csr["chunk_start"], len(csr["chunk_start"])
    n_waves = max(1, -(-csr["total"] // rows_per_wave))
    off = set(np.searchsorted(cs, np.arange(n_waves) * rows_per_wave, side="left").tolist()) | {0}
    empties = [i for i in range(1, n_chunks - 1) if csr["chunk_cnt"][i] == 0 and csr["chunk_slot"][i] < 0]
    off |= {empties[len(empties) // 2], empties[len(empties) // 3] + 1}
    off = sorted(o_ for o_ in off if o_ < n_chunks)
    off.insert(len(off) // 2, off[len(off) // 2])
    return np.asarray(off + [n_chunks], np.int32)


@gpu
@pytest.mark.parametrize("rows_per_wave,total_mod", [(8, 1), (300, 37)])
@pytest.mark.parametrize("W", [256, 512, 768, 1024, 1280, 1536])
def test_segment_sum_stream_guarded(W, rows_per_wave, total_mod):
    """seg_sum_stream_kernel<SLABS, HALF> + seg_finish_kernel at all six widths: a total of 64 k + 1 rows and one that is no multiple of
    8 (64 k + 37); waves of about 8 rows and of about 300 (a range of more than 128 rows: the second block of row ids); empty nodes in
    front, in the middle, at the end, at the start and at the end of a wave's range; an empty wave; a heavy node with an empty chunk."""
    from gtos_amd._lib import call, ptr, stream
    d = dev()
    rng = np.random.RandomState(W + rows_per_wave)
    counts = [0, 0] + rng.choice([0, 1, 1, 1, 2, 3, 5, 17, 63, 64, 150, 700], size=120).tolist() + [130, 0, 3, 0]
    counts += [(total_mod - sum(counts)) % 64, 0]
    csr = make_csr(counts, empty_chunk_in=len(counts) - 6)
    assert csr["total"] % 64 == total_mod
    c = seg_case(d, csr, W, 1, True, W + total_mod, ld_gap=64)
    wave_off = wave_offsets(csr, rows_per_wave)
    call("gtos_segment_sum_stream", len(csr["chunk_node"]), csr["total"], ptr(c["rows"]), ptr(c["cn"]), ptr(c["cs"]), ptr(c["cc"]), ptr(c["sl"]),
         ptr(t32(wave_off, d)), len(wave_off) - 1, ptr(c["src"][0]), c["ld"], W, ptr(c["dst"][0].view), c["ld"], ptr(c["heavy"][0].view), stream())
    seg_finish_and_check("segment_sum_stream W=%d rows/wave=%d total=%d" % (W, rows_per_wave, csr["total"]), csr, c, W)


@gpu
@pytest.mark.parametrize("W", [8, 1528])
def test_segment_sum_ranges_guarded(W):
    """seg_sum_range_kernel<1|3>: an empty range (zeros), ranges of 1 and of 300 rows, overlapping ranges, two blocks of segments"""
    from gtos_amd._lib import call, ptr, stream
    d = dev()
    ranges = [(17, 17), (0, 1), (5, 305), (300, 400), (1, 3), (399, 400), (0, 0), (100, 164), (2, 7)]
    src = guarded_operand(rnd((400, W), BF, W).to(d), ld=W + 8)
    dst = Guarded(len(ranges), W, BF, d, ld=W + 16, init=SENT)
    call("gtos_segment_sum_ranges", len(ranges), ptr(t32(np.asarray(ranges).reshape(-1), d)), ptr(src), W + 8, W, ptr(dst.view), W + 16, stream())
    dst.check("segment_sum_ranges W=%d" % W)
    rows = torch.cat([torch.arange(a, b) for a, b in ranges]).to(d)
    node = torch.cat([torch.full((b - a,), s, dtype=torch.long) for s, (a, b) in enumerate(ranges)]).to(d)
    ref, bound = segment_sum_bounds(src.double()[rows], node, len(ranges))
    assert_within("segment_sum_ranges W=%d" % W, dst.view, ref, bound)
    assert bool((dst.view[0] == 0).all() and (dst.view[6] == 0).all()), "an empty range gives zeros"


@gpu
def test_segment_sum_finish_into_a_wider_matrix():
    """seg_finish_kernel as the relation-attention backward calls it: width 128 into rows of ld_dst = 192 -- the heavy slots rounded once
    (bitwise heavy.to(bf16)), every other row and the 64 columns behind each row untouched"""
    from gtos_amd._lib import call, ptr, stream
    d = dev()
    hn = [7, 0, 3, 11, 9]
    heavy = guarded_operand(rnd((len(hn), 128), F32, 4, 30.0).to(d))
    dst = Guarded(12, 128, BF, d, ld=192, init=SENT)
    call("gtos_segment_sum_finish", len(hn), ptr(t32(hn, d)), ptr(heavy), 128, ptr(dst.view), 192, stream())
    dst.check("segment_sum_finish")
    assert same_bits(dst.view[torch.tensor(hn, device=d)], heavy.to(BF)), "the heavy rows are heavy.to(bf16)"
    rest = torch.ones(12, dtype=torch.bool, device=d)
    rest[torch.tensor(hn, device=d)] = False
    assert untouched(dst.view[rest])
    print("MEASURED segment_sum_finish: %d elements bitwise" % (len(hn) * 128))


@gpu
def test_segment_sums_refuse_bad_widths_and_misaligned_pointers():
    """-24 and nothing written: widths that are no multiple of 8 (256 for the streaming kernel) or above 1536, a leading dimension that
    is no multiple of 8, source or destination pointers off a 16-byte boundary"""
    from gtos_amd._lib import ptr, stream
    d = dev()
    csr = make_csr(SEG_COUNTS)
    c = seg_case(d, csr, 256, 1, True, 1)
    src, dst, heavy = c["src"][0], c["dst"][0], c["heavy"][0]
    n_chunks, wo = len(csr["chunk_node"]), t32([0, len(csr["chunk_node"])], d)

    def rows_args(W, s=0, t=0, ld=c["ld"]):
        return (n_chunks, ptr(c["rows"]), ptr(c["cn"]), ptr(c["cs"]), ptr(c["cc"]), ptr(c["sl"]), ptr(src) + s, None, ld, W,
                ptr(dst.view) + t, None, ld, ptr(heavy.view), None, stream())

    def stream_args(W, s=0, t=0):
        return (n_chunks, csr["total"], ptr(c["rows"]), ptr(c["cn"]), ptr(c["cs"]), ptr(c["cc"]), ptr(c["sl"]), ptr(wo), 1, ptr(src) + s,
                c["ld"], W, ptr(dst.view) + t, c["ld"], ptr(heavy.view), stream())
    for a in (rows_args(12), rows_args(0), rows_args(1544), rows_args(256, s=2), rows_args(256, t=2), rows_args(256, ld=c["ld"] + 4)):
        refuses("-24", "gtos_segment_sum_rows", *a)
    for a in (stream_args(264), stream_args(8), stream_args(1792), stream_args(256, s=2), stream_args(256, t=2)):
        refuses("-24", "gtos_segment_sum_stream", *a)
    rg = t32([0, 5, 5, 9], d)
    for W, s, t in ((12, 0, 0), (1544, 0, 0), (256, 2, 0), (256, 0, 2)):
        refuses("-24", "gtos_segment_sum_ranges", 2, ptr(rg), ptr(src) + s, c["ld"], W, ptr(dst.view) + t, c["ld"], stream())
    refuses("-24", "gtos_segment_sum_finish", c["nh"], ptr(c["hn"]), ptr(heavy.view), 12, ptr(dst.view), c["ld"], stream())
    refuses("-24", "gtos_segment_sum_finish", c["nh"], ptr(c["hn"]), ptr(heavy.view), 256, ptr(dst.view), c["ld"] + 4, stream())
    dst.check("refused segment sums dst")
    heavy.check("refused segment sums heavy")
    assert untouched(dst.view) and bool((heavy.view == 0).all())
