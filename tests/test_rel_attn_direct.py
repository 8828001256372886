"""The streaming relation-attention kernels (gtos_amd/csrc/rel_attn.hip) one call at a time, against float64, inside guard bands.

Four kernels (forward, query-major backward, key-major backward, bank gradient), three relation operands (mode 0 none, mode 1 dense
rarb, mode 2 bank + type ids), seven head widths in lanes (LH = 1 .. 64: every step of head_sum), the fast and the generic lane map,
fp32 and bf16.  Every case calls the C entry points directly, the way ops.RelAttnFn does, with
  * every output a view of a NaN-filled allocation (tests_support.Guarded: bands compared bitwise after each launch, and an element
    of an output that no kernel wrote is still NaN),
  * q, k, v and dq, dk, dv channel slices of [T,B,3d] (self-attention layout) or [T,B,d] + [S,B,2d] (cross layout) row buffers with NaN
    in the leading-dimension gap and in the rows around, NaN bank rows beyond R, and guard entries around every integer array (type ids
    that select a NaN bank row, pair ids that select a NaN key row, chunk records that would store into the band of d_bank),
  * every output held to tests_support.rel_attn_ref / rel_attn_bounds: first-order error propagation from c_acc, C_OUT and c_fast, no
    free tolerance.
GTOS_ATTN_TILE=0 (module fixture) keeps bf16 mode 0 on the streaming kernels.

The CPU self-checks at the top run a plain fp32 emulation (bf16 where the kernels store bf16) through the same comparison: the honest
emulation passes every bound at every small shape of the GPU tests, and each of twelve planted mistakes is rejected."""
import collections
import random

import numpy as np
import pytest
import torch

from tests_support import (Guarded, GuardedFlat, NAN_BITS, _bits, assert_within, c_acc, guarded_operand, lse_comparable,
                           rel_attn_bounds, rel_attn_ref, stored_bound, within_ratio)

gpu = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF]
P_DROP = 0.3


@pytest.fixture(autouse=True)
def _streaming_path(monkeypatch):
    monkeypatch.setenv("GTOS_ATTN_TILE", "0")


def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    return torch.device("cuda:0")


def pow2ceil(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def geometry(d, H):
    """geometry() of rel_attn.hip: (LH, heads per slice, lanes per key row, slices, generic, key groups per wave G, keys per step KS)"""
    hd = d // H
    generic = not (d <= 512 and d & (d - 1) == 0 and hd & (hd - 1) == 0)
    if not generic:
        LH, nhs, lr, slices = hd // 8, H, d // 8, 1
    else:
        LH = pow2ceil(hd // 8)
        nhs = min(64 // LH, pow2ceil(H))
        lr, slices = nhs * LH, -(-H // nhs)
    G = 64 // lr
    return LH, nhs, lr, slices, generic, G, 4 * G


def test_geometry_restatement_covers_every_lane_width_and_both_maps():
    assert [geometry(d, H)[0] for d, H in FAST[:7]] == [1, 2, 4, 8, 16, 32, 64]
    assert geometry(8, 1)[5] == 64 and geometry(512, 8)[5:] == (1, 4) and geometry(32, 4)[6] == 64
    assert not any(geometry(d, H)[4] for d, H in FAST) and all(geometry(d, H)[4] for d, H in GENERIC)
    assert geometry(48, 6)[1:4] == (8, 8, 1) and geometry(96, 4)[:3] == (4, 4, 16)           # idle heads; hd = 24: idle lanes
    assert geometry(640, 5)[:4] == (16, 4, 64, 2) and geometry(1536, 3)[:4] == (64, 1, 64, 3)
    assert geometry(768, 12)[:4] == (8, 8, 64, 2) and geometry(1024, 8)[:4] == (16, 4, 64, 2)


# ------------------------------------------------------------------------------------------------ the cases
# masks: "none" | "pad" (ragged key padding; one fully padded graph when B > 1) | "causal" (plus one fully masked query row) | "both"
# index (mode 2): "host" (relindex.build_relation_index: flagged singletons, 128-pair chunks) | "host-noxcd" (the same, xcd_off null) |
#                 "device" (the fallback of ops.FactoredRelation: no flags, 32-pair chunks) | "hip" (relindex_hip, == host)
Spec = collections.namedtuple("Spec", "mode d H T S B masks p_drop need_w with_dw index ld_extra R layout")
FAST = [(8, 1), (16, 1), (32, 1), (128, 2), (256, 2), (512, 2), (512, 1), (64, 8), (512, 8)]
GENERIC = [(48, 6), (96, 4), (640, 5), (768, 12), (1024, 8), (1536, 3)]
DROPS = [(0.0, False, False), (0.0, True, False), (0.0, True, True), (P_DROP, False, False), (P_DROP, True, False), (P_DROP, True, True)]
MASKS = ["none", "pad", "causal", "both"]
INDEXES = ["host", "device", "host-noxcd"]


def _specs():
    rng = random.Random(20240607)
    out, k = [], 0
    for d, H in FAST + GENERIC:                                 # every lane width, both lane maps, in every mode
        for mode in (0, 1, 2):
            n = [7, 13, 20, 33][(k + k // 4) % 4] if d <= 512 else [5, 9, 12][k % 3]
            T = n - 3 if (mode == 0 and k % 2) else n           # mode 0: cross layout every other case
            p, need_w, with_dw = DROPS[k % 6]
            out.append(Spec(mode, d, H, T, n, [1, 3, 8, 11, 16][k % 5], MASKS[(k + k // 5) % 4], p, need_w, with_dw,
                            INDEXES[(k // 3) % 3], 8 if (k // 3) % 2 else 0, 60, "plain"))
            k += 1
    for d, H in ((32, 4), (512, 8)):                            # key counts against the block's slot KS
        KS = geometry(d, H)[6]
        for S in (1, KS - 1, KS, KS + 1, 2 * KS + 1, 4 * KS + 3):
            for mode in (0, 1, 2):
                T = S if (mode or S <= 20) else 6
                B = [1, 3, 8][k % 3] if S <= 70 else 1
                p, need_w, with_dw = DROPS[(k + 1) % 6]
                out.append(Spec(mode, d, H, T, S, B, MASKS[rng.randrange(4)], p, need_w, with_dw, INDEXES[(k // 3) % 3], 0, 60, "plain"))
                k += 1
    out.append(Spec(0, 128, 2, 1, 37, 3, "pad", 0.0, True, False, None, 0, 0, "plain"))          # the decode step
    out.append(Spec(0, 64, 8, 5, 70, 11, "both", P_DROP, True, True, None, 0, 0, "plain"))
    return out


SMALL = _specs()
N_SHAPE_CASES = 3 * len(FAST + GENERIC)
SMALL_CASES = [(s, dt) for i, s in enumerate(SMALL) for dt in DTYPES
               if i < N_SHAPE_CASES or i >= N_SHAPE_CASES + 36 or dt == DTYPES[(i // 3 + s.mode) % 2]]
# mode 2 on crafted type ids: every index form, xcd_off given and null, B = 3 and B = 8 with one XCD left without chunks, and more chunks
# (R = 17000, mostly absent types) than the capped grid of the bank kernel takes in one pass
INDEX_CASES = [Spec(2, 64, 8, 20, 20, 3, "pad", 0.0, False, False, ix, 8, 60, "plain") for ix in ("host", "host-noxcd", "device", "hip")] + [
    Spec(2, 64, 8, 20, 20, 8, "pad", P_DROP, True, True, "host", 0, 480, "host_empty"),
    Spec(2, 64, 8, 20, 20, 8, "both", 0.0, False, False, "device", 8, 60, "device_empty"),
    Spec(2, 32, 4, 20, 20, 3, "pad", 0.0, False, False, "host", 8, 17000, "plain"),
    Spec(2, 32, 4, 20, 20, 3, "none", 0.0, False, False, "host-noxcd", 0, 17000, "plain")]
BIG = [Spec(0, 8, 1, 1025, 1025, 1, "both", P_DROP, True, True, None, 0, 0, "plain"),
       Spec(1, 8, 1, 1025, 1025, 1, "both", 0.0, True, True, None, 0, 0, "plain"),
       Spec(2, 8, 1, 1025, 1025, 1, "both", P_DROP, False, False, "host", 8, 60, "plain")]
BIG_DTYPES = [BF, F32, BF]                                      # mode 1 in fp32: rarb is 67 MB


def sid(s):
    return "m%d-d%d-H%d-T%d-S%d-B%d-%s-p%g-w%d-dw%d-%s-R%d" % (s.mode, s.d, s.H, s.T, s.S, s.B, s.masks, s.p_drop, s.need_w, s.with_dw,
                                                             s.index if s.mode == 2 else "x", s.R)


def did(dt):
    return "bf16" if dt == BF else "fp32"


def case_id(v):
    return sid(v[0]) + "-" + did(v[1])


def hash_keep(seed, n, p):
    from test_hip_parity import _hash_keep
    return _hash_keep(seed, np.arange(n, dtype=np.uint64), p)


COUNTS = [1, 1, 1, 1, 2, 32, 33, 64, 65, 128, 129, 300]


def craft_relation(n, B, R, seed, key_pad, layout):
    """relation[j,i,b] type ids in [0,R), crafted: absent types (0, 5 and the last ones among them), four singletons (the first on a padded
    key when there is one), types with exactly 2, 32, 33, 64, 65, 128, 129 and 300 pairs as far as the n*n*B pairs allow, the rest spread
    over a few filler types.  Returns (relation, info) with info = dict(absent=..., singles=..., counts={type: pairs}).
    layout "host_empty" (B = 8): every type with more than one pair lives in ONE of the graphs 0..6 and graph 7 holds singletons only, so
    the host index has no chunk for XCD 7; "device_empty" (B = 8): graphs 0 and 7 are one single type whose 32-pair chunks all start on a
    pair of graph 0, everything else lives in graphs 1..6, so the device-derived index has no chunk for XCD 7."""
    g = torch.Generator().manual_seed(seed)
    P = n * n * B
    rel = torch.full((n * n, B), -1, dtype=torch.long)
    absent = sorted({0, 5, R - 1, R - 2, R - 4} & set(range(R))) if R > 12 else []
    ids = [t for t in range(1, R) if t not in absent]
    order = [ids[i] for i in torch.randperm(len(ids), generator=g).tolist()] if R <= 100 else ids
    graphs = list(range(B))
    if layout == "host_empty":
        assert B == 8 and R >= 60 + n * n + 6
        block = list(range(60, 60 + n * n))                    # graph 7: one singleton type per pair, ids 60 .. 60 + n*n - 1
        rel[:, 7] = torch.tensor(block)[torch.randperm(n * n, generator=g)]
        order = [t for t in order if t < 59] + [59] + list(range(60 + n * n, R - 4))
        graphs = list(range(7))
    elif layout == "device_empty":
        assert B == 8
        t0 = order.pop(0)
        rel[:, 0] = t0
        rel[:, 7] = t0
        graphs = list(range(1, 7))
    free = {b: torch.randperm(n * n, generator=g).tolist() for b in graphs}
    info = dict(absent=absent, singles=[], counts={})

    def take(cnt, one_graph):
        if one_graph:
            b = max(graphs, key=lambda x: len(free[x]))
            if len(free[b]) < cnt:
                return None
            return [(free[b].pop(), b) for _ in range(cnt)]
        if sum(len(v) for v in free.values()) < cnt:
            return None
        got = []
        while len(got) < cnt:
            b = graphs[int(torch.randint(0, len(graphs), (1,), generator=g))]
            if free[b]:
                got.append((free[b].pop(), b))
        return got

    first_single = layout != "host_empty"
    for cnt in COUNTS:
        if not order:
            break
        where = None
        if cnt == 1 and first_single and key_pad is not None and bool(key_pad.any()):
            for j, b in torch.nonzero(key_pad).tolist():        # the first singleton sits on a padded key (its bank row must come back 0)
                if b in free and j * n in free[b]:
                    free[b].remove(j * n)
                    where = [(j * n, b)]
                    break
        first_single = first_single and cnt != 1
        where = where or take(cnt, layout == "host_empty")
        if where is None:
            continue
        t = order.pop(0)
        for ji, b in where:
            rel[ji, b] = t
        info["counts"][t] = cnt
        if cnt == 1:
            info["singles"].append(t)
    if layout == "host_empty":
        info["singles"] += block
    fill = order[:25] if layout != "host_empty" else order
    for b in graphs:                                            # the rest: filler types (host_empty: each filler type in one graph)
        mine = fill[b::len(graphs)] if layout == "host_empty" else fill
        if free[b]:
            mine = torch.tensor(mine if mine else info["singles"][:1])
            rel[torch.tensor(free[b]), b] = mine[torch.randint(0, len(mine), (len(free[b]),), generator=g)]
    assert int(rel.min()) >= 0
    present = set(rel.unique().tolist())
    info["absent"] = [t for t in range(R) if t not in present]
    cnts = torch.bincount(rel.reshape(-1), minlength=R)
    info["singles"] = torch.nonzero(cnts == 1).flatten().tolist()
    return rel.reshape(n, n, B), info


class Case(object):
    pass


def make_case(spec, dtype, device):
    """The stored operands of one case on ``device`` (contiguous; the GPU tests copy them into guarded buffers)."""
    c = Case()
    c.spec, c.dtype = spec, dtype
    mode, d, H, T, S, B = spec.mode, spec.d, spec.H, spec.T, spec.S, spec.B
    hd = d // H
    g = torch.Generator().manual_seed(1000003 * d + 1009 * S + 31 * T + 7 * B + mode)

    def rnd(shape, scale=1.0, dt=dtype):
        return (torch.randn(shape, generator=g) * scale).to(dt).to(device)
    c.q, c.k, c.v, c.d_o = rnd((T, B, d)), rnd((S, B, d)), rnd((S, B, d)), rnd((T, B, d))
    c.scale = hd ** -0.5
    c.d_w = rnd((T, S, B, H), hd ** 0.5, F32) if spec.with_dw else None      # comparable to d_o . v
    c.key_pad = c.attn_mask = None
    if spec.masks in ("pad", "both"):
        lens = torch.randint(max(1, S // 2), S + 1, (B,), generator=g)
        if B > 1:
            lens[1] = 0                                                       # one fully padded graph
        elif S > 1:
            lens[0] = S - 1
        c.key_pad = (torch.arange(S)[:, None] >= lens[None, :]).to(torch.uint8)
    if spec.masks in ("causal", "both"):
        m = torch.triu(torch.ones(T, S), 1).bool()
        m[min(2, T - 1), :] = True                                            # one fully masked query row
        c.attn_mask = m.to(torch.uint8)
    c.rel = c.relation = c.info = None
    c.R = spec.R
    if mode == 1:
        c.rel = rnd((S, T, B, 2 * d), 0.5)
    elif mode == 2:
        c.relation, c.info = craft_relation(S, B, spec.R, 17 + S + B, c.key_pad, spec.layout)
        c.rel = rnd((spec.R, 2 * d), 0.5)
        c.relation = c.relation.to(device)
    c.seed = 0x9E3779B97F4A7C15 ^ (d * 65537 + S)                            # both halves of the 64-bit seed in use
    c.keep = None
    if spec.p_drop > 0:
        c.keep = hash_keep(c.seed, T * S * B * H, spec.p_drop).reshape(T, S, B, H).to(device)
    if c.key_pad is not None:
        c.key_pad = c.key_pad.to(device)
    if c.attn_mask is not None:
        c.attn_mask = c.attn_mask.to(device)
    return c


def reference(c):
    s = c.spec
    ref = rel_attn_ref(c.q, c.k, c.v, s.H, c.scale, s.mode, c.rel, c.relation, c.R, c.key_pad, c.attn_mask, s.p_drop, c.keep, c.d_o, c.d_w)
    G, KS = geometry(s.d, s.H)[5:]
    return ref, rel_attn_bounds(ref, c.dtype, KS, G, with_w=s.need_w)


def names_of(spec):
    return ["o", "lse"] + (["w"] if spec.need_w else []) + ["pd", "gs", "dq", "dk", "dv"] + (["d_rel"] if spec.mode else [])


def ratios(c, got, ref, bounds):
    out = {}
    for name in names_of(c.spec):
        g, r = got[name].reshape(ref[name].shape), ref[name]
        if name == "lse":
            g, r = lse_comparable(g, r)
        out[name] = within_ratio(g, r, bounds[name])[0]
    return out


def check_all(tag, c, got, ref, bounds):
    for name in names_of(c.spec):
        g, r = got[name].reshape(ref[name].shape), ref[name]
        if name == "lse":
            g, r = lse_comparable(g, r)
        assert_within("rel_attn %s %s" % (tag, name), g, r, bounds[name])


# ------------------------------------------------------------------------------------------------ fp32 emulation and planted mistakes
MUTATIONS = ["key dropped from the softmax sum", "rb omitted from dq", "ra omitted from dk", "d_rel halves swapped", "scale missing from gs",
             "D without the w.dw term", "keep with i and j exchanged", "keep_scale twice on o", "pair left out of a bank row",
             "singleton bank row unwritten", "absent bank row unwritten", "lse of a masked row finite"]
ONLY_MODES = {"rb omitted from dq": (1, 2), "ra omitted from dk": (1, 2), "d_rel halves swapped": (1, 2), "pair left out of a bank row": (2,),
              "singleton bank row unwritten": (2,), "absent bank row unwritten": (2,)}


def emulate(c, mutate=None):
    """Forward and backward in plain fp32 torch on the stored operands, rounded to the stored type where the kernels store it (o, dq, dk,
    dv, d_rel); the backward reads the rounded o and the fp32 lse / w as the kernels do.  ``mutate``: one planted mistake."""
    s = c.spec
    mode, d, H, T, S, B = s.mode, s.d, s.H, s.T, s.S, s.B
    hd, dt, scale = d // H, c.dtype, float(c.scale)
    q5, k5 = c.q.float().reshape(T, 1, B, H, hd), c.k.float().reshape(1, S, B, H, hd)
    v4, do4 = c.v.float().reshape(S, B, H, hd), c.d_o.float().reshape(T, B, H, hd)
    full = (T, S, B, H, hd)
    if mode == 0:
        qa, kb, ra, rb = q5.expand(full), k5.expand(full), None, None
    else:
        rows = c.rel.float() if mode == 1 else c.rel.float()[c.relation]
        rows = rows.reshape(S, T, B, 2 * d).permute(1, 0, 2, 3)
        ra, rb = rows[..., :d].reshape(full), rows[..., d:].reshape(full)
        qa, kb = q5 + ra, k5 + rb
    sc = (qa * kb).sum(-1) * scale
    dead = torch.zeros(T, S, B, 1, dtype=torch.bool)
    if c.key_pad is not None:
        dead = dead | c.key_pad.bool().reshape(1, S, B, 1)
    if c.attn_mask is not None:
        dead = dead | c.attn_mask.bool().reshape(T, S, 1, 1)
    dead = dead.expand(T, S, B, H)
    sm = sc.masked_fill(dead, float("-inf"))
    m = sm.amax(1, keepdim=True)
    has = torch.isfinite(m)
    m0 = torch.where(has, m, torch.zeros_like(m))
    e = torch.exp(sm - m0)
    l = e.sum(1, keepdim=True)
    if mutate == "key dropped from the softmax sum":
        l = l - e.gather(1, (~dead).int().argmax(1, keepdim=True))           # the first live key of every row
    p = e * torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    lse = torch.where(has, m0 + torch.log(l), torch.full_like(m, 0.0 if mutate == "lse of a masked row finite" else float("-inf"))).squeeze(1)
    ks = float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(s.p_drop))) if s.p_drop > 0 else 1.0
    keep = torch.ones(T, S, B, H) if c.keep is None else c.keep.float()
    if mutate == "keep with i and j exchanged":
        keep = keep.transpose(0, 1).contiguous()                              # the mask of counter ((j S + i) B + b) H + h
    kf = keep * ks
    w = p * kf
    o = torch.einsum("ijbh,jbhe->ibhe", w, v4).reshape(T, B, d)
    if mutate == "keep_scale twice on o":
        o = o * ks
    o_st = o.to(dt)
    dw = torch.zeros_like(w) if c.d_w is None else c.d_w.float()
    D = (do4 * o_st.float().reshape(T, B, H, hd)).sum(-1)
    if mutate != "D without the w.dw term":
        D = D + (w * dw).sum(1)
    pb = torch.where(dead | ~has, torch.zeros_like(sc), torch.exp(sc - lse[:, None]))
    pd = w if s.need_w else pb * kf                                           # the forward's weights when it returned them
    gs = pb * (kf * (torch.einsum("ibhe,jbhe->ijbh", do4, v4) + dw) - D[:, None])
    if mutate != "scale missing from gs":
        gs = gs * scale
    dq = torch.einsum("ijbh,ijbhe->ibhe", gs, k5.expand(full) if mutate == "rb omitted from dq" else kb).reshape(T, B, d)
    dk = torch.einsum("ijbh,ijbhe->jbhe", gs, q5.expand(full) if mutate == "ra omitted from dk" else qa).reshape(S, B, d)
    dv = torch.einsum("ijbh,ibhe->jbhe", pd, do4).reshape(S, B, d)
    got = dict(o=o_st, lse=lse, w=w, pd=pd, gs=gs, dq=dq.to(dt), dk=dk.to(dt), dv=dv.to(dt))
    if mode:
        halves = [(gs[..., None] * kb).reshape(T, S, B, d), (gs[..., None] * qa).reshape(T, S, B, d)]
        if mutate == "d_rel halves swapped":
            halves.reverse()
        pair = torch.cat(halves, -1).permute(1, 0, 2, 3)
        if mode == 1:
            got["d_rel"] = pair.to(dt)
        else:
            tid = c.relation.reshape(-1)
            rows = pair.reshape(-1, 2 * d).clone()
            if mutate == "pair left out of a bank row":
                t = max(c.info["counts"], key=lambda x: (c.info["counts"][x] <= 33, c.info["counts"][x]))      # the 33- (or 32-, 2-) pair type
                live = torch.nonzero((tid == t) & (rows.abs().sum(1) > 0)).flatten()
                rows[live[0]] = 0.0
            bank = torch.zeros(c.R, 2 * d).index_add_(0, tid, rows)
            if mutate == "singleton bank row unwritten":
                bank[c.info["singles"][-1]] = float("nan")                    # the band pattern it was allocated with
            if mutate == "absent bank row unwritten":
                bank[c.info["absent"][0]] = float("nan")
            got["d_rel"] = bank.to(dt)
    return got


ACCEPT_CASES = SMALL_CASES + [(s, dt) for s in INDEX_CASES[4:6] for dt in DTYPES]


@pytest.mark.parametrize("spec,dtype", ACCEPT_CASES, ids=[case_id(v) for v in ACCEPT_CASES])
def test_bounds_accept_the_honest_emulation(spec, dtype):
    c = make_case(spec, dtype, "cpu")
    ref, bounds = reference(c)
    check_all("emulated " + case_id((spec, dtype)), c, emulate(c), ref, bounds)


REJECT_SPECS = {0: Spec(0, 64, 8, 13, 13, 3, "both", P_DROP, True, True, None, 0, 0, "plain"),
                1: Spec(1, 128, 2, 13, 13, 3, "both", P_DROP, True, True, None, 0, 0, "plain"),
                2: Spec(2, 96, 4, 20, 20, 3, "both", P_DROP, True, True, "host", 0, 60, "plain")}


@pytest.mark.parametrize("dtype", DTYPES, ids=did)
@pytest.mark.parametrize("mutate,mode", [(mu, mo) for mu in MUTATIONS for mo in ONLY_MODES.get(mu, (0, 1, 2))])
def test_bounds_reject(mutate, mode, dtype):
    c = make_case(REJECT_SPECS[mode], dtype, "cpu")
    ref, bounds = _reject_reference(mode, dtype, c)
    r = ratios(c, emulate(c, mutate), ref, bounds)
    print("MUTATION %s (mode %d, %s): err/bound %s" % (mutate, mode, did(dtype), {k: "%.3g" % v for k, v in r.items()}))
    assert max(r.values()) > 1.0, r


_REJECT_REFS = {}


def _reject_reference(mode, dtype, c):
    if (mode, dtype) not in _REJECT_REFS:                                     # one reference per (mode, dtype), shared by the mutations
        _REJECT_REFS[(mode, dtype)] = reference(c)
    return _REJECT_REFS[(mode, dtype)]


def test_crafted_relation_has_every_kind_of_type():
    rel, info = craft_relation(20, 3, 60, 1, torch.arange(20)[:, None] >= torch.tensor([20, 0, 15])[None, :], "plain")
    cnt = torch.bincount(rel.reshape(-1), minlength=60)
    assert set(COUNTS) <= set(cnt.tolist()) and int((cnt == 1).sum()) >= 3 and int((cnt == 0).sum()) >= 3 and cnt[59] == 0
    on_pad = [(j, b) for j, i, b in torch.nonzero(cnt[rel] == 1).tolist() if b == 1 or (b == 2 and j >= 15)]
    assert on_pad, "one singleton sits on a padded key"
    from gtos_amd.relindex import build_relation_index
    ix = build_relation_index(rel, 60)
    assert int(ix.chunk_count.max()) == 128 and ix.n_heavy >= 6               # the sb loop of the bank kernel: chunks above 64 pairs
    assert not (set(ix.chunk_type.tolist()) & set(info["singles"])) and bool((ix.idx_q < 0).any())      # singletons: flagged, no chunk
    rel8, _ = craft_relation(20, 8, 480, 2, None, "host_empty")
    ix8 = build_relation_index(rel8, 480)
    assert bool((ix8.xcd_off[1:] == ix8.xcd_off[:-1]).any()), ix8.xcd_off.tolist()      # an XCD without chunks
    big, _ = craft_relation(20, 3, 17000, 3, None, "plain")
    assert build_relation_index(big, 17000).nchunks > 16384                   # past the capped grid: the chunk walk strides


# ------------------------------------------------------------------------------------------------ on the GPU
def _p(t, off=0):
    return None if t is None else t.data_ptr() + off * t.element_size()


def int_guard(t, fill, pad=64):
    """int32 array with ``pad`` guard entries ``fill`` in front and behind"""
    buf = torch.full((2 * pad + t.numel(),), fill, dtype=torch.int32, device=t.device)
    view = buf[pad:pad + t.numel()]
    view.copy_(t.reshape(-1))
    return view


def is_band(t):
    return bool((_bits(t) == NAN_BITS[t.dtype]).all())


class Launch(object):
    """The guarded buffers of one case and the three launches."""

    def __init__(self, c, index=None):
        s = c.spec
        self.c = c
        T, S, B, H, d, dt = s.T, s.S, s.B, s.H, s.d, c.dtype
        dv_, N = dev(), s.T * s.S * s.B * s.H
        tr = max(8, B + 1)
        if T == S:                                                            # self-attention layout: q | k | v in one [T,B,3d] buffer
            ld = 3 * d + 8
            buf = guarded_operand(torch.cat([c.q, c.k, c.v], -1).reshape(T * B, 3 * d), ld=ld, trail=tr)
            self.q, self.k, self.v = (_p(buf, i * d) for i in range(3))
            self.ldq = self.ldk = self.ldv = ld
            self.gq = self.gkv = Guarded(T * B, 3 * d, dt, dv_, ld=ld, lead=8, trail=8)
            self.gq.regions = []
            self.dq, self.dk, self.dv = (self.gq.carve(self.gq.base + i * d, T * B, d, ld) for i in range(3))
        else:                                                                 # cross layout: q alone, k | v in one [S,B,2d] buffer
            qb = guarded_operand(c.q.reshape(T * B, d), ld=d + 8, trail=tr)
            kv = guarded_operand(torch.cat([c.k, c.v], -1).reshape(S * B, 2 * d), ld=2 * d + 8, trail=tr)
            buf = (qb, kv)
            self.q, self.k, self.v, self.ldq, self.ldk, self.ldv = _p(qb), _p(kv), _p(kv, d), d + 8, 2 * d + 8, 2 * d + 8
            self.gq = Guarded(T * B, d, dt, dv_, ld=d + 8, lead=8, trail=8)
            self.gkv = Guarded(S * B, 2 * d, dt, dv_, ld=2 * d + 8, lead=8, trail=8)
            self.gkv.regions = []
            self.dq = self.gq.view
            self.dk, self.dv = (self.gkv.carve(self.gkv.base + i * d, S * B, d, 2 * d + 8) for i in range(2))
        self.hold = [buf]
        self.rel = self.idx_q = self.idx_k = None
        self.R = c.R
        if s.mode == 1:
            self.rel = guarded_operand(c.rel.reshape(S * T * B, 2 * d))
        elif s.mode == 2:
            self.rel = guarded_operand(c.rel)                                 # NaN rows beyond R: where a guard id points
            self.index = index
            self.idx_q, self.idx_k = int_guard(index["idx_q"], self.R, max(64, S)), int_guard(index["idx_k"], self.R, max(64, T))
        self.d_o = guarded_operand(c.d_o.reshape(T * B, d), ld=d + 8)
        self.o = Guarded(T * B, d, dt, dv_, lead=8, trail=8)
        self.lse = Guarded(T * B, H, F32, dv_, lead=8, trail=8)
        self.w = GuardedFlat(N, F32, dv_) if s.need_w else None
        self.pd, self.gs = GuardedFlat(N, F32, dv_), GuardedFlat(N, F32, dv_)
        self.d_w = None if c.d_w is None else GuardedFlat(N, F32, dv_, init=c.d_w.reshape(1, -1)).view
        self.d_rel, self.ld_drel = None, 0
        if s.mode == 1:
            self.d_rel = Guarded(S * T * B, 2 * d, dt, dv_, lead=8, trail=8)
        elif s.mode == 2:
            self.ld_drel = 2 * d + s.ld_extra
            self.d_rel = Guarded(self.R, 2 * d, dt, dv_, ld=self.ld_drel, lead=8, trail=8)
        self.common = (s.mode, T, S, B, H, d, self.q, self.ldq, self.k, self.ldk, self.v, self.ldv, _p(self.rel))

    def guards(self):
        return [(n, g) for n, g in (("o", self.o), ("lse", self.lse), ("w", self.w), ("pd", self.pd), ("gs", self.gs), ("dq buffer", self.gq),
                                    ("dk / dv buffer", self.gkv), ("d_rel", self.d_rel), ("heavy", getattr(self, "heavy", None))) if g is not None]

    def check(self, when):
        for n, g in self.guards():
            g.check("%s: %s" % (when, n))

    def forward(self):
        from gtos_amd._lib import call, dt, stream
        c, s = self.c, self.c.spec
        call("gtos_rel_attn_fwd", dt(c.q), *self.common, _p(self.idx_q), _p(c.key_pad), _p(c.attn_mask), float(c.scale), float(s.p_drop),
             c.seed, _p(self.o.view), s.d, _p(self.lse.view), _p(self.w.view) if self.w else None, stream())
        self.check("after the forward")

    def backward(self, pd=True, d_w="case", w="case", ld_drel=None):
        from gtos_amd._lib import call, dt, stream
        c, s = self.c, self.c.spec
        d_w = self.d_w if d_w == "case" else d_w
        w = (self.w.view if self.w else None) if w == "case" else w
        call("gtos_rel_attn_bwd", dt(c.q), *self.common, _p(self.idx_q), _p(self.idx_k), _p(c.key_pad), _p(c.attn_mask), float(c.scale),
             float(s.p_drop), c.seed, _p(self.o.view), s.d, _p(self.lse.view), _p(w), _p(self.d_o), s.d + 8, _p(d_w),
             _p(self.dq), self.ldq, _p(self.dk), self.ldk, _p(self.dv), self.ldv, _p(self.d_rel.view) if self.d_rel else None,
             self.ld_drel if ld_drel is None else ld_drel, _p(self.pd.view) if pd else None, _p(self.gs.view) if pd else None, stream())
        self.check("after the backward")

    def bank(self, xcd=True, ld=None):
        from gtos_amd._lib import call, dt, stream
        c, s, ix = self.c, self.c.spec, self.index
        P, nh = s.S * s.S * s.B, int(ix["heavy_types"].numel())
        self.heavy = Guarded(max(nh, 1), 2 * s.d, F32, dev(), lead=8, trail=8, init=0.0)
        arrays = [int_guard(ix["pair_sorted"], P), int_guard(ix["chunk_type"], self.R), int_guard(ix["chunk_start"], P),
                  int_guard(ix["chunk_count"], 1), int_guard(ix["chunk_slot"], -1)]
        xo = ix["xcd_off"].to(torch.int32).contiguous() if xcd else None
        call("gtos_rel_attn_bwd_bank", dt(c.q), s.S, s.B, s.H, s.d, self.q, self.ldq, self.k, self.ldk, _p(self.rel), _p(self.gs.view),
             *[_p(a) for a in arrays], _p(xo), int(ix["nchunks"]), _p(self.d_rel.view), self.ld_drel if ld is None else ld,
             _p(self.heavy.view), stream())
        self.check("after the bank gradient")
        if nh and ld is None:
            ht = ix["heavy_types"].to(torch.int32).contiguous()
            if c.dtype == BF:
                call("gtos_segment_sum_finish", nh, _p(ht), _p(self.heavy.view), 2 * s.d, _p(self.d_rel.view), self.ld_drel, stream())
                self.check("after the heavy rows' fold")
            else:
                self.d_rel.view[ht.long()] = self.heavy.view[:nh]

    def outputs(self):
        s = self.c.spec
        torch.cuda.synchronize()
        got = dict(o=self.o.view, lse=self.lse.view, pd=self.pd.view, gs=self.gs.view, dq=self.dq, dk=self.dk, dv=self.dv)
        if self.w:
            got["w"] = self.w.view
        if self.d_rel:
            got["d_rel"] = self.d_rel.view
        return got


def build_index(c, kind):
    """the arrays of the bank-gradient pass as a dict of device tensors"""
    names = ("idx_q", "idx_k", "pair_sorted", "chunk_type", "chunk_start", "chunk_count", "chunk_slot", "xcd_off", "heavy_types", "nchunks")
    if kind in ("host", "host-noxcd", "hip"):
        from gtos_amd.relindex import build_relation_index
        ix = build_relation_index(c.relation.cpu(), c.R).to(dev())
        if kind == "hip":
            from gtos_amd.relindex_hip import HipBackend, build_relation_index_staged
            from test_pathtrie import _same_object
            staged = build_relation_index_staged(c.relation, c.R, HipBackend.shared())
            torch.cuda.synchronize()
            assert _same_object(ix.cpu(), staged.cpu()) == [], "the device builder's arrays are the host builder's"
            ix = staged
    else:
        from gtos_amd import ops
        with torch.enable_grad():
            ix = ops.FactoredRelation(torch.zeros(c.R, 8, device=dev()), c.relation)
        assert int(ix.idx_q.min()) >= 0 and int(ix.chunk_count.max()) <= 32  # no flags, 32-pair chunks
    return {n: getattr(ix, n) for n in names}


def run_case(spec, dtype):
    c = make_case(spec, dtype, dev())
    index = build_index(c, spec.index) if spec.mode == 2 else None
    if spec.layout.endswith("_empty"):
        xo = index["xcd_off"]
        assert bool((xo[1:] == xo[:-1]).any()), "the case is built to leave one XCD without chunks: %s" % xo.tolist()
    run = Launch(c, index)
    run.forward()
    run.backward()
    if spec.mode == 2:
        run.bank(xcd=spec.index != "host-noxcd")
    got = run.outputs()
    ref, bounds = reference(c)
    tag = case_id((spec, dtype))
    if spec.need_w:
        diff = int((_bits(got["pd"]) != _bits(got["w"])).sum())
        print("MEASURED rel_attn %s pd vs w: %d of %d elements differ in their bits" % (tag, diff, got["w"].numel()))
    check_all(tag, c, got, ref, bounds)
    if spec.need_w:
        assert torch.equal(_bits(got["pd"]), _bits(got["w"])), "pd (backward) and w (forward) differ in their bits"
    if spec.mode == 2:
        absent = torch.tensor(c.info["absent"], dtype=torch.long, device=dev())
        assert absent.numel() > 0 and float(got["d_rel"][absent].float().abs().max()) == 0.0, "a type without pairs has a zero row"
    return c, got, ref


@gpu
@pytest.mark.parametrize("spec,dtype", SMALL_CASES, ids=[case_id(v) for v in SMALL_CASES])
def test_every_output_within_its_bound(spec, dtype):
    """every lane width and both lane maps in every mode; key counts around the block's slot; T != S; masks, dropout, w and dw spread
    over them"""
    run_case(spec, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=did)
@pytest.mark.parametrize("spec", INDEX_CASES, ids=sid)
def test_mode2_index_forms_within_their_bounds(spec, dtype):
    """crafted type ids (absent types, singletons, 2 .. 300 pairs per type) under the host index, the device-derived one and the device
    builder's; xcd_off given and null; an XCD without chunks; more chunks than the capped grid takes in one pass"""
    c, got, ref = run_case(spec, dtype)
    assert len(c.info["singles"]) >= 3 and len(c.info["absent"]) >= 3
    if spec.R >= 17000:
        assert int(build_index(c, spec.index)["nchunks"]) > 16384


@gpu
@pytest.mark.parametrize("spec,dtype", list(zip(BIG, BIG_DTYPES)), ids=[case_id(v) for v in zip(BIG, BIG_DTYPES)])
def test_more_than_1024_keys_within_the_bounds(spec, dtype):
    """S = T = 1025: masks and type ids are read from global memory, not staged in LDS"""
    run_case(spec, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=did)
def test_refusals_leave_the_outputs_untouched(dtype):
    from gtos_amd._lib import GtosHipError
    from gtos_amd._lib import call, dt, stream

    def untouched(run):
        run.check("after a refused call")
        torch.cuda.synchronize()
        for n, g in run.guards():
            if n != "heavy":
                assert is_band(g.buf), n

    # -12: a relation operand with T != S
    c = make_case(Spec(1, 64, 8, 9, 9, 3, "none", 0.0, False, False, None, 0, 0, "plain"), dtype, dev())
    run = Launch(c)
    run.common = (1, 8, 9) + run.common[3:]
    with pytest.raises(GtosHipError, match="-12"):
        run.forward()
    with pytest.raises(GtosHipError, match="-12"):
        run.backward()
    untouched(run)
    # -13: dw without w;  -15: the streaming backward without pd / gs
    c = make_case(Spec(0, 64, 8, 9, 9, 3, "none", 0.0, True, True, None, 0, 0, "plain"), dtype, dev())
    run = Launch(c)
    with pytest.raises(GtosHipError, match="-13"):
        run.backward(w=None)
    with pytest.raises(GtosHipError, match="-15"):
        run.backward(pd=False)
    untouched(run)
    # -14: ld_drel below 2d or no multiple of 8, at both entry points
    c = make_case(Spec(2, 64, 8, 9, 9, 3, "none", 0.0, False, False, "host", 8, 60, "plain"), dtype, dev())
    run = Launch(c, build_index(c, "host"))
    for ld in (2 * 64 - 8, 2 * 64 + 4):
        with pytest.raises(GtosHipError, match="-14"):
            run.backward(ld_drel=ld)
        with pytest.raises(GtosHipError, match="-14"):
            run.bank(ld=ld)
    untouched(run)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=did)
def test_attention_core_mode2_bank_gradient_end_to_end(dtype):
    """ops.attention_core with the host index and heavy types, two layers that share one bank through ops.linear and a GradAccumGroup
    (bf16: the layers' d_rel are column blocks of one slab, ld_drel = 4d, and the heavy rows are folded by gtos_segment_sum_finish).
    The projections are the two halves of the bank (weights [I | 0] and [0 | I]), so bank.grad is the two d_rel side by side."""
    from gtos_amd import ops
    from gtos_amd.relindex import build_relation_index
    spec = Spec(2, 64, 8, 20, 20, 3, "pad", 0.0, False, False, "host", 0, 60, "plain")
    d, H, n, B, R = spec.d, spec.H, spec.S, spec.B, spec.R
    layers = [make_case(spec._replace(T=n, S=n), dtype, dev()) for _ in range(2)]
    g = torch.Generator().manual_seed(99)
    layers[1].q = (torch.randn(n, B, d, generator=g)).to(dtype).to(dev())     # the second layer: its own queries and upstream gradient
    layers[1].d_o = (torch.randn(n, B, d, generator=g)).to(dtype).to(dev())
    bank = torch.cat([layers[0].rel, (0.5 * torch.randn(R, 2 * d, generator=g)).to(dtype).to(dev())], 1).requires_grad_()
    layers[1].rel = bank.detach()[:, 2 * d:].contiguous()
    eye = torch.eye(4 * d, device=dev(), dtype=dtype)
    index = build_relation_index(layers[0].relation.cpu(), R).to(dev())
    assert index.n_heavy >= 6
    fact = ops.FactoredRelation(bank.detach(), layers[0].relation, index=index)
    rels = [ops.linear(bank, eye[l * 2 * d:(l + 1) * 2 * d], group=fact.grad_group) for l in range(2)]
    loss, qs = 0.0, []
    for c, rel in zip(layers, rels):
        c.rel = rel.detach()                                                  # the stored projection: the bank's half
        qkv = torch.cat([c.q, c.k, c.v], -1).requires_grad_()
        o, _ = ops.attention_core(qkv, None, (0, d, 2 * d), d, H, c.scale, rel=rel, fact=fact, key_pad=c.key_pad)
        loss = loss + (o.float() * c.d_o.float()).sum()
        qs.append((qkv, o))
    loss.backward()
    ops.join_side()
    torch.cuda.synchronize()
    for l, (c, (qkv, o)) in enumerate(zip(layers, qs)):
        ref, bounds = reference(c)
        tag = "attention_core %s layer %d " % (did(dtype), l)
        assert_within(tag + "o", o.detach(), ref["o"], bounds["o"])
        for i, name in enumerate(("dq", "dk", "dv")):
            assert_within(tag + name, qkv.grad[..., i * d:(i + 1) * d], ref[name], bounds[name])
        # the identity product adds nothing in bf16 (exact products, one term per sum); fp32: one more rounding of the GEMM's sum
        got = bank.grad[:, l * 2 * d:(l + 1) * 2 * d]
        assert_within(tag + "bank.grad", got, ref["d_rel"], stored_bound(ref["d_rel"], bounds["d_rel"] + c_acc(4 * d) * ref["d_rel"].abs(), dtype))
        absent = torch.tensor(c.info["absent"], device=dev())
        assert float(got[absent].float().abs().max()) == 0.0
