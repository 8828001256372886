"""Golden results for gtos_amd.metrics, produced by the REFERENCE's own two scoring programs (generator/chrF++.py and
generator/multi-bleu.perl, which generator/work.py's validate calls), run by path and not copied.

  metrics_dev48.json
      refs    the English token line of the first 48 four-line records of translator_data/dev.txt
      hyps    a fixed perturbation of each reference with random.Random(7): per word one draw u -- u < 0.12 drops the word,
              u < 0.20 replaces it by a random word of the sentence, u < 0.25 doubles it; a hypothesis is never left empty
      chrf    what `python chrF++.py -R ref -H hyp -s` prints: the 48 sentence scores, F and avgF
      bleu    the fields of the line `perl multi-bleu.perl ref < hyp` prints

Every sentence pair scores above 0 (asserted): for a pair with F = 0 chrF++.py adds the PREVIOUS sentence's counts to its corpus
totals, which is not a behaviour to pin.

Run in the build container only:  python tests/golden/make_golden_metrics.py
"""
import json
import os
import random
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
N = 48


def perturb(words, rng):
    out = []
    for w in words:
        u = rng.random()
        if u < 0.12:
            continue
        if u < 0.20:
            out.append(rng.choice(words))
        elif u < 0.25:
            out += [w, w]
        else:
            out.append(w)
    return out or [words[0]]


def main():
    lines = open(os.path.join(REF, "translator_data", "dev.txt"), encoding="utf-8").read().split("\n")
    refs = [lines[4 * i + 2].split() for i in range(N)]
    rng = random.Random(7)
    hyps = [perturb(r, rng) for r in refs]
    tdir = tempfile.mkdtemp()
    ref_path, hyp_path = os.path.join(tdir, "ref"), os.path.join(tdir, "hyp")
    for path, sents in ((ref_path, refs), (hyp_path, hyps)):
        with open(path, "w", encoding="utf-8") as fo:
            fo.write("".join(" ".join(s) + "\n" for s in sents))
    out = subprocess.run([sys.executable, os.path.join(REF, "generator", "chrF++.py"), "-R", ref_path, "-H", hyp_path, "-s"],
                         check=True, stdout=subprocess.PIPE).stdout.decode()
    sent = [float(m.group(2)) for m in re.finditer(r"^(\d+)::c6\+w2-F2\t([0-9.]+)$", out, flags=re.M)]
    assert len(sent) == N and min(sent) > 0, "every pair must score above 0"
    chrf = {"sentence": sent, "F": float(re.search(r"^c6\+w2-F2\t([0-9.]+)$", out, flags=re.M).group(1)),
            "avgF": float(re.search(r"^c6\+w2-avgF2\t([0-9.]+)$", out, flags=re.M).group(1))}
    with open(hyp_path, "rb") as fi:
        line = subprocess.run(["perl", os.path.join(REF, "generator", "multi-bleu.perl"), ref_path], check=True, stdin=fi,
                              stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode().strip()
    m = re.match(r"BLEU = ([0-9.]+), ([0-9.]+)/([0-9.]+)/([0-9.]+)/([0-9.]+) \(BP=([0-9.]+), ratio=([0-9.]+), hyp_len=(\d+), ref_len=(\d+)\)", line)
    bleu = {"line": line, "bleu": float(m.group(1)), "precisions": [float(m.group(i)) for i in range(2, 6)], "bp": float(m.group(6)),
            "hyp_len": int(m.group(8)), "ref_len": int(m.group(9))}
    path = os.path.join(HERE, "metrics_dev48.json")
    with open(path, "w", encoding="utf-8") as fo:
        json.dump({"refs": refs, "hyps": hyps, "chrf": chrf, "bleu": bleu}, fo, ensure_ascii=False, sort_keys=True)
        fo.write("\n")
    print(line)
    print("chrF++ F %.4f avgF %.4f, lowest sentence %.4f; metrics_dev48.json %.1f KB"
          % (chrf["F"], chrf["avgF"], min(sent), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
