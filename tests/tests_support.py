"""Shared constants (must match tests/golden/make_golden.py) and helpers of the GPU tests."""
import torch

SMALL_VOCAB = dict(concept=60, token=70, predictable_token=50, relation=26, concept_char=20, token_char=22)
SMALL_GEN_ARGS = (8, 12, 8, 12, [(3, 16)], 10, 10, 6, 8, 2)   # char/word dims, filters, rel_dim, rnn


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
