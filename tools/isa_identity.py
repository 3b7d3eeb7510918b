#!/usr/bin/env python3
"""Is the device assembly of two build trees the same?  For a change that may rename things but must not change a kernel.

    make -C aletsch_amd/csrc isa [ROWS=1 | STARREG=1 | WSYNC=1]        in a checkout of each commit
    python tools/isa_identity.py LABEL PARENT/build/csrc[_rows...] HEAD/build/csrc[_rows...]   >> profiles/rNN/isa_identity.txt

One line per file of isa/ and isa_other/: the hashes of both sides and `same` or `differs`, after dropping the lines that carry only
file names, line numbers or comments.  The files that hold several kernels (isa_other/) are also compared function by function, and
every function of a file that differs is listed.  Exit status 1 if anything differs."""
import glob, hashlib, os, re, sys


def norm(path):
    out = []
    for ln in open(path, errors="replace"):
        t = ln.strip()
        if not t or t.startswith((";", "//", ".file", ".loc", ".ident")):
            continue
        out.append(ln.rstrip())
    return out


def functions(lines):
    """name -> its lines, from the label to .Lfunc_end (what lies between functions -- descriptors, metadata -- is compared with the file)"""
    fs = {}; cur = None
    for ln in lines:
        m = re.match(r"^([A-Za-z_][\w$.]*):", ln)
        if cur is None and m and not ln.startswith(".L") and not m.group(1).endswith(".kd"):
            cur = m.group(1); fs[cur] = []
        if cur:
            fs[cur].append(ln)
            if ln.strip().startswith(".Lfunc_end"):
                cur = None
    return {k: v for k, v in fs.items() if v[-1].strip().startswith(".Lfunc_end")}


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16] if lines is not None else "-" * 16


def main():
    label, parent, head = sys.argv[1:4]
    bad = 0
    for sub in ("isa", "isa_other"):
        for f in sorted(glob.glob(os.path.join(head, sub, "*.s"))):
            name = sub + "/" + os.path.basename(f); g = os.path.join(parent, sub, os.path.basename(f))
            a = norm(g) if os.path.exists(g) else None; b = norm(f)
            same = a == b; bad += not same
            print(f"{label:8s} {name:28s} parent {digest(a)} head {digest(b)} {'same' if same else 'differs'}")
            if a is not None and (sub == "isa_other" or not same):
                fa, fb = functions(a), functions(b)
                for k in sorted(set(fa) | set(fb)):
                    if k.startswith("_ZN7rocprim") or k.startswith("_ZN6hipcub"):
                        if fa.get(k) == fb.get(k):
                            continue                               # library kernels: listed only when they differ
                    print(f"{label:8s}     {k} parent {digest(fa.get(k))} head {digest(fb.get(k))} {'same' if fa.get(k) == fb.get(k) else 'differs'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
