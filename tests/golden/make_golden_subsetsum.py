"""tests/golden/ref_subsetsum_wide.json.gz: subset-sum instances over the whole domain of the kernel (1..32 items a side, bumped items,
dense lists, ties, sort order; tests/subsetsum_cases.py: fixture_selection()), answered by the reference.

Every instance goes to oracle/_ref/ref_subsetsum (the reference's own scallop/subsetsum.cc, built by oracle/Makefile) in a process of its
own, as make_golden.py does: the reference aborts on an instance without a cross pair, and such an instance is stored with the answer null.
The error e is stored as the float its %.17g text parses to.  Instances and answers are stored; nothing else.

    python tests/golden/make_golden_subsetsum.py        (needs oracle/_ref/ref_subsetsum: build() makes it)
"""
import gzip
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import subsetsum_cases as cases  # noqa: E402

OUT = os.path.join(HERE, "ref_subsetsum_wide.json.gz")
MAX_BYTES = 1 << 20


def reference_answer(exe, s, t):
    """one process per instance -> {"e", "s", "t"} or None where the reference aborts"""
    txt = "1\n%d %d\n" % (len(s), len(t)) + " ".join("%d %d" % tuple(p) for p in s) + "\n" + " ".join("%d %d" % tuple(p) for p in t) + "\n"
    r = subprocess.run([exe], input=txt, capture_output=True, text=True)
    if r.returncode != 0 or not r.stdout.strip():
        return None
    f = r.stdout.split(); k = int(f[1]); m = int(f[2 + k])
    return {"e": float(f[0]), "s": [int(x) for x in f[2:2 + k]], "t": [int(x) for x in f[3 + k:3 + k + m]]}


def load():
    """[(family, source, target, answer)] of the stored instances"""
    d = json.loads(gzip.decompress(open(OUT, "rb").read()))
    return [(i["family"], [tuple(x) for x in i["s"]], [tuple(x) for x in i["t"]], a) for i, a in zip(d["instances"], d["answers"])]


def main():
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_subsetsum")
    sel = cases.fixture_selection()
    ans = [reference_answer(exe, s, t) for _, s, t in sel]
    blob = json.dumps({"seed": cases.FIXTURE_SEED, "instances": [{"family": f, "s": s, "t": t} for f, s, t in sel], "answers": ans},
                      separators=(",", ":")).encode()
    z = gzip.compress(blob, 9, mtime=0)
    assert len(z) < MAX_BYTES, len(z)
    open(OUT, "wb").write(z)
    print("ref_subsetsum_wide.json.gz: %d instances, %d refused, %d bytes" % (len(sel), sum(a is None for a in ans), len(z)))


if __name__ == "__main__":
    main()
