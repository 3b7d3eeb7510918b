"""tests/golden/ref_tset_collide.json.gz: the reference's answers for the cases of tests/collide_cases.py, whose chains share hash buckets.

The groups are not stored: collide_cases.groups_of() draws them again from the seed.  What is stored, per case, is what
oracle/_ref/ref_tset (the reference's own rnacore/transcript_set.cc + gtf/transcript.cc, built by oracle/Makefile) prints:

  seq          the groups replayed in order into one set (meta/assembler.cc:1105-1133)
  merge2/3     `ref_tset merge K1 K2 ...`: the groups cut at one half / at thirds, every segment replayed into a set of its own, the sets
               folded left to right with transcript_set::add(transcript_set&) -- two finished sets that both hold items
  seq_multi    seq over the groups without their single-exon transcripts: what skip_single_exon must give

make_golden.tset_parse reads each of them.

    python tests/golden/make_golden_tset_collide.py        (needs oracle/_ref/ref_tset: build() makes it)
"""
import gzip
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))
import collide_cases as cc  # noqa: E402
import make_golden as mg  # noqa: E402

OUT = os.path.join(HERE, "ref_tset_collide.json.gz")
PARTS = (2, 3)
KEYS = ("seq", "merge2", "merge3", "seq_multi")


def ask(exe, groups, parts=1):
    args = ["merge"] + [str(k) for k in cc.segments(len(groups), parts)] if parts > 1 else []
    return subprocess.run([exe] + args, input=mg.tset_text(groups), capture_output=True, text=True, check=True).stdout


def knows_merge(exe):
    """does this build of the driver take `merge K1 K2 ...`?  It refuses segments that do not add up to the groups on stdin (exit status
    2); a build of the driver as it was before it learnt `merge` ignores its arguments and answers as if there were none"""
    return subprocess.run([exe, "merge", "1"], input="0\n", capture_output=True, text=True).returncode == 2


def reference_outputs(exe, merges=True):
    out = []
    for i in range(len(cc.CASES)):
        groups = cc.groups_of(i)
        d = {"seq": ask(exe, groups), "seq_multi": ask(exe, cc.multi_exon_only(groups))}
        for p in PARTS if merges else ():
            d["merge%d" % p] = ask(exe, groups, p)
        out.append(d)
    return out


def stored():
    return json.loads(gzip.decompress(open(OUT, "rb").read()))


def load():
    """[(groups, {key: items})] of the stored cases"""
    d = stored()
    assert d["seed"] == cc.SEED and [tuple(s) for s in d["shapes"]] == list(cc.CASES)
    return [(cc.groups_of(i), {k: mg.tset_parse(o[k]) for k in KEYS}) for i, o in enumerate(d["out"])]


def main():
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_tset")
    assert knows_merge(exe), "oracle/_ref/ref_tset was built from an earlier driver: make -C oracle"
    outs = reference_outputs(exe)
    blob = json.dumps({"seed": cc.SEED, "shapes": cc.CASES, "out": outs}).encode()
    open(OUT, "wb").write(gzip.compress(blob, 9, mtime=0))
    print("ref_tset_collide.json.gz: %d cases, %s items, %d bytes" % (len(outs), [len(mg.tset_parse(o["seq"])) for o in outs], os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
