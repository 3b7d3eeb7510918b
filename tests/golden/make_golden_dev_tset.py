"""tests/golden/ref_tset_resident.json.gz: larger transcript-set cases for the resident (device) set, answered by the reference.

Each case is a long run of transcript groups (one group = one graph) drawn from few intron chains, so later groups keep landing on
items that much earlier ones made -- the coverage of such an item is summed across many calls in the reference's nesting.  The groups
are not stored: resident_groups() draws them again from the seed (make_golden.tset_case).  What is stored is the merged set as
oracle/_ref/ref_tset (the reference's own rnacore/transcript_set.cc + gtf/transcript.cc, built by oracle/Makefile) prints it,
replaying meta/assembler.cc:1105-1133; make_golden.tset_parse reads it.

    python tests/golden/make_golden_dev_tset.py        (needs oracle/_ref/ref_tset: build() makes it)
"""
import gzip
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

OUT = os.path.join(HERE, "ref_tset_resident.json.gz")
SEED = 2026
SHAPES = ((2000, 8, 60), (10000, 8, 120))          # (groups, samples, intron chains)


def resident_groups():
    rng = random.Random(SEED)
    return [mg.tset_case(rng, ng, ns, nc) for ng, ns, nc in SHAPES]


def reference_outputs(exe):
    return [subprocess.run([exe], input=mg.tset_text(g), capture_output=True, text=True, check=True).stdout for g in resident_groups()]


def load():
    """[(groups, items)] of the stored cases"""
    d = json.loads(gzip.decompress(open(OUT, "rb").read()))
    return [(g, mg.tset_parse(out)) for g, out in zip(resident_groups(), d["out"])]


def main():
    outs = reference_outputs(os.path.join(ROOT, "oracle", "_ref", "ref_tset"))
    blob = json.dumps({"seed": SEED, "shapes": SHAPES, "out": outs}).encode()
    open(OUT, "wb").write(gzip.compress(blob, 9, mtime=0))
    print("ref_tset_resident.json.gz: %d cases, %d items" % (len(outs), sum(len(mg.tset_parse(o)) for o in outs)))


if __name__ == "__main__":
    main()
