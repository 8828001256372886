"""Teacher-forced scoring at the model level, on the GPU: Generator.score against the pinned oracle's ll row, against Generator.forward,
against the scores the device beam search gives its own hypotheses, and Trainer.evaluate in front of a training step.  (The kernels,
the host glue and the dry-run plans are in tests/test_score_eval.py.)"""
import numpy as np
import pytest
import torch

from conftest import load_golden, sub

pytestmark = pytest.mark.gpu

FP32 = dict(rtol=1e-3, atol=1e-3)         # the project's fp32 parity bar
NEAR = 1e-5
NEAR_SHARE = 0.01


def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    return torch.device("cuda:0")


def to_dev(d):
    return {k: (v.to(dev()) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def oracle_ll_row(om, data):
    """The oracle's forward in eval mode up to TokenGenerator(work=True): ll [T,B,C] (oracle/gtos_oracle.py Generator.forward with
    the decoder asked for the row instead of the loss)."""
    from oracle import gtos_oracle as O
    with torch.no_grad():
        graph, gmask, probe = om.encode_step(data, train=False)
        T = data['token_in'].shape[0]
        pos = O.sinusoid_table(max(T, 2), om.embed_dim)[:T].unsqueeze(1)
        tok = om.embed_scale * om.token_encoder(data['token_in'], data['token_char_in']) + pos
        tok = om.token_embed_layer_norm(tok)
        tmask = data['token_in'].eq(om.vocabs['token'].padding_idx)
        amask = O.causal_mask(T)
        tok = om.snt_encoder(tok, self_padding_mask=tmask, self_attn_mask=amask, external_memories=graph, external_padding_mask=gmask)
        return om.decoder(probe.expand_as(tok), graph, tok, gmask, tmask, amask, data['cp_seq'], work=True)


def lowest_argmax(ll):
    cols = torch.arange(ll.shape[-1]).expand_as(ll)
    return torch.where(ll == ll.max(-1, keepdim=True).values, cols, ll.shape[-1]).min(-1).values


def oracle_scores(om, data, pad=0):
    ll = oracle_ll_row(om, data).double()
    y = data['token_out']
    live = y.ne(pad)
    token_ll = ll.gather(-1, y.unsqueeze(-1)).squeeze(-1).masked_fill(~live, 0.0)
    top2 = ll.topk(2, dim=-1).values
    near = (top2[..., 0] != top2[..., 1]) & ((top2[..., 0] - top2[..., 1]) < NEAR)      # |log p1 - log p2| < 1e-5: p within 1e-5 relative
    return token_ll, lowest_argmax(ll), near, live


@pytest.mark.parametrize("name", ["gen_small", "gen_padded"])
@pytest.mark.parametrize("which", ["batch/", "ebatch/"])
def test_score_vs_oracle_fp32(name, which):
    from test_hip_parity import build_generator
    from test_oracle_golden import build_small_generator
    g = load_golden(name)
    m = build_generator(g, True)
    om = build_small_generator(g)
    om.eval()
    data = sub(g, which)
    want_ll, want_pred, near, live = oracle_scores(om, data)
    assert float(near.double().mean()) <= NEAR_SHARE, "%d near ties among the oracle's %d rows" % (int(near.sum()), near.numel())
    for mode in (True, False):
        m.train(mode)
        sc = m.score(to_dev(data))
        assert m.training == mode
        torch.testing.assert_close(sc.token_ll.cpu().double(), want_ll, **FP32)
        bad = (sc.pred.cpu().long() != want_pred) & ~near
        assert not bool(bad.any()), (sc.pred.cpu()[bad], want_pred[bad])
        assert sc.tokens.cpu().tolist() == live.sum(0).tolist()
        assert sc.correct.cpu().tolist() == ((sc.pred.cpu().long() == data['token_out']) & live).sum(0).tolist()
        torch.testing.assert_close(sc.sentence_ll.cpu(), sc.token_ll.cpu().double().sum(0), rtol=1e-12, atol=1e-12)
        assert sc.graph_of.cpu().tolist() == list(range(live.shape[1]))
    # label smoothing does not enter a score
    from gtos_amd.decoder import set_label_smoothing
    set_label_smoothing(m, 0.1)
    assert torch.equal(m.score(to_dev(data)).token_ll, sc.token_ll)


@pytest.mark.parametrize("name", ["gen_small", "gen_padded"])
def test_score_bf16_sentence_ll_close(name):
    from test_hip_parity import build_generator
    from test_oracle_golden import build_small_generator
    g = load_golden(name)
    m = build_generator(g, True)
    m.set_compute_dtype(torch.bfloat16)
    om = build_small_generator(g)
    om.eval()
    data = sub(g, "batch/")
    want = oracle_scores(om, data)[0].sum(0)
    got = m.score(to_dev(data)).sentence_ll.cpu()
    print("MEASURED bf16 sentence_ll", got.tolist(), want.tolist())
    assert bool(((got - want).abs() <= 1e-2 * want.abs().clamp(min=1.0)).all()), (got, want)      # the bf16 loss bar


@pytest.mark.parametrize("name", ["gen_small", "gen_padded"])
def test_forward_is_the_reference_normalised_mean_of_score(name):
    from test_hip_parity import build_generator
    g = load_golden(name)
    m = build_generator(g, True)
    m.eval()
    data = to_dev(sub(g, "batch/"))
    assert data['relation'].dim() == 3
    with torch.no_grad():
        loss = float(m(data))
    sc = m.score(data)
    mean = float((-sc.sentence_ll / sc.tokens.double()).mean())
    print("MEASURED forward %.9g vs score %.9g" % (loss, mean))
    assert abs(loss - mean) <= 1e-6 * abs(mean)


def _beam_model(case, tmp_path):
    from test_beam_and_vocab import load_case, make_vocabs, batch_of, state_dict_of
    from gtos_amd.generator import Generator
    meta, arrs = load_case(case)
    vocabs = make_vocabs(meta, tmp_path)
    cfg = meta["cfg"]
    ga = [[tuple(f) for f in a] if isinstance(a, list) else a for a in cfg["gen_args"]]
    model = Generator(vocabs, *ga, cfg["d"], cfg["ff"], cfg["H"], 0.0, cfg["snt_layers"], cfg["graph_layers"],
                      cfg["inference_layers"], None, dev(), depth_size=cfg.get("depth_size", 32)).to(dev())
    model.load_state_dict(state_dict_of(arrs))
    model.eval()
    return model, batch_of(meta, arrs, dev()), meta, vocabs


@pytest.mark.parametrize("case", ["beam_smatch", "beam_dep_dev"])
def test_score_agrees_with_the_device_beam_search(case, tmp_path):
    """Per token the incremental decoder and the teacher-forced pass are the same function: every finished hypothesis of
    work(search="device"), passed back as an n-best list per graph, scores as the search scored it, |diff| <= 1e-3 (tokens + 1)."""
    from gtos_amd.vocab import END
    model, batch, meta, _ = _beam_model(case, tmp_path)
    alpha = meta["cfg"]["alpha"]
    compared = 0
    for run in meta["runs"]:
        beams = model.work(batch, run["beam"], run["max_step"], run["min_step"], search="device")
        hyps = [beam.get_k_best(run["beam"], alpha) for beam in beams]
        targets = [[list(h.seq[1:-1]) if h.seq[-1] == END else list(h.seq[1:]) for h in hs] for hs in hyps]
        sc = model.score(batch, targets)
        ll, tokens, owner = sc.sentence_ll.cpu().tolist(), sc.tokens.cpu().tolist(), sc.graph_of.cpu().tolist()
        flat = [(b, h) for b, hs in enumerate(hyps) for h in hs]
        assert len(flat) == len(ll) and owner == [b for b, _ in flat]
        for (b, h), got, n in zip(flat, ll, tokens):
            if h.seq[-1] != END:                  # unfinished: scored (with an <END> the search never took), not compared
                continue
            assert n == len(h.seq) - 1
            assert abs(got - h.score) <= 1e-3 * (n + 1), (case, run["beam"], b, h.seq, got, h.score)
            compared += 1
    assert compared > 0


def test_score_of_the_batchs_own_sentences_given_as_strings(tmp_path):
    from gtos_amd.vocab import END
    model, batch, meta, vocabs = _beam_model("beam_dep_dev", tmp_path)
    cv, pad = vocabs['token_char'], vocabs['predictable_token'].padding_idx
    tch, tout = batch['token_char_in'].cpu(), batch['token_out'].cpu()
    sents = []
    for n in range(tout.shape[1]):           # the strings, from the character rows of the inputs (row t + 1 spells target t)
        L = int(tout[:, n].ne(pad).sum()) - 1
        words = []
        for t in range(1, L + 1):
            chars = cv.idx2token(tch[t, n].tolist())
            words.append("".join(chars[1:chars.index(END)]))
        sents.append(words)
    own = model.score(batch)
    given = model.score(batch, sents)
    assert given.graph_of.cpu().tolist() == list(range(tout.shape[1]))
    assert own.tokens.cpu().tolist() == given.tokens.cpu().tolist()
    a, b = own.sentence_ll.cpu(), given.sentence_ll.cpu()
    print("MEASURED own vs strings", a.tolist(), b.tolist())
    assert bool(((a - b).abs() <= 1e-5 * a.abs()).all())
    assert torch.equal(own.pred, given.pred)
    strings = given.strings(batch)
    assert [len(s) for s in strings] == given.tokens.cpu().tolist() and all(isinstance(w, str) for s in strings for w in s)


def _fresh_trainer(dtype):
    from gtos_amd import ops, synth
    from gtos_amd.config import generator_args
    from gtos_amd.generator import Generator
    from gtos_amd.pathtrie import attach_path_trie
    from gtos_amd.relindex import attach_relation_index
    from gtos_amd.train import Trainer
    cfg = synth.CONFIGS["C1"]
    torch.manual_seed(19940117)
    model = Generator(synth.synth_vocabs(), device=dev(), **generator_args(cfg)).to(dev())
    model.set_compute_dtype(dtype)
    model.train()
    trainer = Trainer(model, cfg["d"], warmup_steps=2000, compute_dtype=dtype, world_size=1, rank=0)
    ops.set_seed(424242)
    batches = []
    for i in range(3):
        b, _ = synth.make_config_batch("C1", rank=i, padded=(i == 1))
        batches.append({k: v.to(dev()) for k, v in attach_relation_index(attach_path_trie(b)).items()})
    return trainer, batches


def _check_evaluate_in_place(trainer, batches):
    """evaluate() on ``batches``: every piece of training state bitwise as before, metrics consistent with the batches"""
    from gtos_amd import ops
    flat, dev_ = trainer.flat, trainer.flat.param.device
    mirror = getattr(flat, "mirror", None)
    before = (flat.param.clone(), flat.grad.clone(), flat.m.clone(), flat.v.clone(), None if mirror is None else mirror.clone(),
              trainer._state.clone(), ops._seed_state[0], trainer.steps_issued, [m.training for m in trainer.model.modules()])
    assert not ops._DW_PENDING.get(dev_)
    res = trainer.evaluate(batches)
    torch.cuda.synchronize()
    assert not ops._DW_PENDING.get(dev_)
    after = (flat.param, flat.grad, flat.m, flat.v, mirror, trainer._state)
    for x, y in zip(before[:6], after):
        assert (x is None and y is None) or torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert ops._seed_state[0] == before[6] and trainer.steps_issued == before[7]
    assert [m.training for m in trainer.model.modules()] == before[8]
    assert res["tokens"] == sum(int(b['token_out'].ne(0).sum()) for b in batches)
    assert res["sentences"] == sum(b['token_out'].shape[1] for b in batches)
    assert 0.0 <= res["accuracy"] <= 1.0 and res["nll_per_token"] > 0 and np.isfinite(res["loss"])
    assert abs(res["perplexity"] - np.exp(res["nll_per_token"])) <= 1e-9 * res["perplexity"]
    return res


@pytest.mark.parametrize("name", ["gen_small", "gen_padded"])
def test_evaluate_leaves_training_bitwise_untouched(name):
    """Two fresh identical Trainers, same seeds; one evaluates two batches (the training batch's K-path eval twin among them) before
    its step.  Afterwards parameters, Adam moments, loss and counters are BITWISE equal and the model is in train mode.
    The configuration is the golden-pinned small model in bf16 because its training step is reproducible from run to run (measured:
    4 runs x 2 steps bit-identical); the same model in fp32 and the synthetic C1 in either precision are not -- their backward sums
    with floating-point atomics (two identical runs WITHOUT any evaluation differed by up to 6e-8 in the parameters) -- so a bitwise
    comparison after a step says nothing about evaluate() there.  test_evaluate_does_not_touch_trainer_state_c1 covers those sizes
    by comparing the state around evaluate() itself."""
    from test_hip_parity import build_generator
    from gtos_amd import ops
    from gtos_amd.train import Trainer
    g = load_golden(name)
    d = int(g["cfg"][0])
    states = []
    for with_eval in (True, False):
        m = build_generator(g, True)
        m.set_compute_dtype(torch.bfloat16)
        m.train()
        trainer = Trainer(m, d, warmup_steps=10, compute_dtype=torch.bfloat16)
        ops.set_seed(424242)
        batch, ebatch = to_dev(sub(g, "batch/")), to_dev(sub(g, "ebatch/"))
        if with_eval:
            _check_evaluate_in_place(trainer, [ebatch, batch])
        loss = trainer.step(batch)
        loss2 = trainer.step(batch)
        torch.cuda.synchronize()
        states.append((trainer.flat.param.clone(), trainer.flat.m.clone(), trainer.flat.v.clone(), (loss, loss2), trainer.counters(),
                       ops._seed_state[0], trainer.model.training))
    a, b = states
    for i, what in enumerate(("parameters", "Adam m", "Adam v")):
        assert torch.equal(a[i].view(torch.int32), b[i].view(torch.int32)), what + " differ after an evaluation in front of the step"
    assert a[3] == b[3] and a[4] == b[4] and a[5] == b[5] and a[6] and b[6]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_evaluate_does_not_touch_trainer_state_c1(dtype):
    trainer, batches = _fresh_trainer(dtype)
    trainer.step(batches[0])                      # (a trainer in mid-training: moments and counters are not zero)
    _check_evaluate_in_place(trainer, batches[1:])
    assert trainer.model.training
    v = trainer.step(batches[0])
    torch.cuda.synchronize()
    assert v is None or np.isfinite(v)
