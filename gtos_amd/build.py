"""Builds libgtos_hip.so (gfx950) in-tree with hipcc.  No torch in the build: the library is plain C ABI."""
import os
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB = os.path.join(CSRC, "libgtos_hip.so")
SOURCES = ["gemm.hip", "rel_attn.hip", "attn_tile.hip", "rowops.hip", "gru_step.hip", "copy_nll.hip", "tokenenc.hip", "pathtrie_dev.hip", "relbatch_dev.hip", "relindex_dev.hip", "beam.hip", "sample.hip", "copy_ls.hip", "copy_eval.hip", "copy_explain.hip", "ngram.hip", "diverse.hip", "constrain.hip", "coverage.hip", "phrase.hip", "avoid.hip", "sbs.hip", "truncate.hip", "overlap.hip", "mbr.hip"]
EXACT_FP = {"relbatch_dev.hip", "beam.hip", "sample.hip", "diverse.hip", "constrain.hip", "coverage.hip", "phrase.hip", "sbs.hip", "truncate.hip"}      # double comparisons / sums that must come out like the host code: no fast-math, no contraction
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffast-math", "-fno-finite-math-only"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _deps(obj, fallback):
    """Headers the object was compiled from, read from the depfile its last compilation wrote (-MMD); without one, the headers the
    source is known to include.  Only headers inside the repository are tracked (the ROCm headers do not change under us)."""
    dfile = obj[:-2] + ".d"
    root = os.path.dirname(os.path.dirname(CSRC))
    try:
        words = open(dfile).read().replace("\\\n", " ").split()
    except OSError:
        return fallback
    deps = [w for w in words[1:] if w.endswith((".h", ".hpp")) and os.path.abspath(w).startswith(root) and os.path.exists(w)]
    return deps or fallback


HOST_SRCS = [os.path.join(os.path.dirname(CSRC), "csrc_host", f) for f in ("relbatch.cpp", "pathtrie.cpp", "relindex.cpp")]
HOST_LIB = os.path.join(os.path.dirname(CSRC), "csrc_host", "libgtos_host.so")
CXX = os.environ.get("CXX", "g++")


def build_host(force=False, verbose=True):
    """libgtos_host.so: the C++ graph -> relation-tensor path (include/gtos_host.h); plain g++, no GPU code."""
    hdr = os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "gtos_host.h")
    shared = [os.path.join(CSRC, h) for h in ("relbatch_kernels.h", "relindex_kernels.h", "trie_kernels.h")]   # stage code the host and GPU builders share
    if force or _stale(HOST_LIB, HOST_SRCS + [hdr] + shared):
        cmd = [CXX, "-O3", "-std=c++17", "-shared", "-fPIC", "-pthread"] + HOST_SRCS + ["-o", HOST_LIB]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return HOST_LIB


def build(force=False, verbose=True):
    build_host(force, verbose)
    own_hdr = {"pathtrie_dev.hip": "trie_kernels.h", "relbatch_dev.hip": "relbatch_kernels.h",
               "relindex_dev.hip": "relindex_kernels.h", "beam.hip": "beam_kernels.h beam_device.h slot_kernels.h slot_device.h reorder_device.h",
               "sample.hip": "sample_kernels.h slot_kernels.h slot_device.h",
               "sbs.hip": "sbs_kernels.h sample_kernels.h beam_kernels.h slot_kernels.h slot_device.h common.h", "copy_ls.hip": "copy_ls_kernels.h",
               "copy_nll.hip": "copy_row.h", "rel_attn.hip": "common.h attn_tile.h", "attn_tile.hip": "common.h attn_tile.h",
               "copy_eval.hip": "copy_eval_kernels.h", "copy_explain.hip": "copy_row.h copy_explain_kernels.h copy_eval_kernels.h",
               "ngram.hip": "common.h ngram_kernels.h slot_kernels.h",
               "avoid.hip": "common.h avoid_kernels.h slot_kernels.h",
               "overlap.hip": "common.h overlap_kernels.h slot_kernels.h",
               "mbr.hip": "common.h mbr_kernels.h overlap_kernels.h slot_kernels.h",
               "truncate.hip": "truncate_kernels.h sample_kernels.h slot_kernels.h slot_device.h common.h",
               "diverse.hip": "diverse_kernels.h beam_kernels.h beam_device.h slot_kernels.h slot_device.h reorder_device.h",
               "constrain.hip": "constrain_kernels.h beam_kernels.h beam_device.h slot_kernels.h slot_device.h common.h",
               "coverage.hip": "coverage_kernels.h beam_kernels.h beam_device.h slot_kernels.h slot_device.h common.h",
               "phrase.hip": "phrase_kernels.h constrain_kernels.h beam_kernels.h beam_device.h slot_kernels.h slot_device.h common.h"}     # the others include common.h
    objs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + _deps(o, [os.path.join(CSRC, h) for h in own_hdr.get(src, "common.h").split()])):
            flags = [f for f in FLAGS if f not in ("-ffast-math", "-fno-finite-math-only")] + ["-ffp-contract=off"] if src in EXACT_FP else FLAGS
            cmd = [HIPCC] + flags + ["-MMD", "-MF", o[:-2] + ".d", "-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
    if force or _stale(LIB, objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", LIB]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
