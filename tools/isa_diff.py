"""Is the device code of two checkouts the same?  Per kernel symbol, from the compiler's own assembly (no GPU needed).

usage: python tools/isa_diff.py OLD_TREE NEW_TREE [file.hip ...]        (no files: every .hip of NEW_TREE's csrc/)
       ... --moved OLD.hip=NEW1.hip,NEW2.hip,...     OLD.hip of OLD_TREE against the union of the symbols of NEW_TREE's NEW*.hip: the proof of a split.  A
                                                     symbol several of them carry (a static kernel of a shared header) must have the same text in each.

Each file is compiled in both trees with the Makefile's CXXFLAGS plus --cuda-device-only -S, once plain and once with -DVS_DET_BUILD=1.  Every function symbol
gets one verdict:
  identical    the same text (body, kernel descriptor, metadata entry; .file / .ident lines dropped)
  equivalent   the same count of every mnemonic, the same value of every .amdhsa_* directive and the same metadata entry (register, spill, LDS, scratch and
               kernarg sizes): what a refactor that only moved source into helpers may leave behind, e.g. scalar moves that traded places or register numbers
  DIFFERENT    anything else
A file's symbols are listed unless all of them are identical; then its summary line stands for them.
Exit status 1 on any DIFFERENT and on any symbol that only one tree has.  What it is for: proving that shared helpers compile to the code the copies
compiled to.  It classifies no instruction: it compares whatever mnemonics it finds.
"""
import collections
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("vae_segmentation_amd", "csrc")


def parse(asm):
    """assembly text -> {symbol: {"text": [lines], "ops": Counter, "hsa": {directive: value}, "meta": [lines]}}"""
    lines = [ln.rstrip() for ln in asm.split("\n") if not re.match(r"^\s*\.(file|ident)\b", ln)]
    syms = collections.OrderedDict()
    entry = lambda: {"text": [], "ops": collections.Counter(), "hsa": {}, "meta": []}
    funcs = set(m.group(1) for ln in lines for m in [re.match(r"^\s*\.type\s+([\w.$]+),\s*@function", ln)] if m)
    cur = where = None
    for ln in lines:
        s = ln.strip()
        m = re.match(r"^([\w.$]+):", s)
        if where is None and m and (m.group(1) in funcs or not funcs and not s.startswith(".")):
            cur, where = syms.setdefault(m.group(1), entry()), "body"
        elif where is None and s.startswith(".amdhsa_kernel"):
            cur, where = syms.setdefault(s.split()[1], entry()), "hsa"
        elif where is None and s.startswith(".amdgpu_metadata"):
            where = "meta"
            cur = None
            continue
        if where == "body":
            cur["text"].append(ln)
            code = s.split(";")[0].strip()
            if code.startswith(".size") or code.startswith(".section"):
                where = None
            elif code and not code.startswith(".") and not code.endswith(":"):
                cur["ops"][code.split()[0]] += 1
        elif where == "hsa":
            cur["text"].append(ln)
            if s.startswith(".end_amdhsa_kernel"):
                where = None
            elif s.startswith(".amdhsa_") and not s.startswith(".amdhsa_kernel"):
                cur["hsa"][s.split()[0]] = " ".join(s.split()[1:])
        elif where == "meta":
            if s.startswith(".end_amdgpu_metadata"):
                where = None
            elif re.match(r"^  - \.", ln):                     # a new entry of amdhsa.kernels
                cur = []
                cur.append(ln)
            elif cur is not None and ln.startswith("    "):
                cur.append(ln)
                m = re.match(r"^    \.name:\s+(\S+)", ln)
                if m:
                    syms.setdefault(m.group(1).strip("'\""), entry())["meta"] = cur
            else:
                cur = None
    for e in syms.values():
        e["text"] = e["text"] + e["meta"]
    return syms


def compare(asm_a, asm_b):
    """-> {symbol: "identical" | "equivalent" | "DIFFERENT" | "only in old" | "only in new"}"""
    return compare_moved(asm_a, [asm_b])


def compare_moved(asm_old, asms_new):
    """compare() of one old file against the union of the files its code moved into.  A symbol that several new files carry (a static kernel of a shared
    header) counts once and must have the same text in each: copies that differ are DIFFERENT, whatever the old file held."""
    a, b, clash = parse(asm_old), collections.OrderedDict(), set()
    for asm in asms_new:
        for k, e in parse(asm).items():
            if b.setdefault(k, e)["text"] != e["text"]:
                clash.add(k)
    out = collections.OrderedDict()
    for k in list(a) + [k for k in b if k not in a]:
        if k in clash:
            out[k] = "DIFFERENT"
        elif k not in b:
            out[k] = "only in old"
        elif k not in a:
            out[k] = "only in new"
        elif a[k]["text"] == b[k]["text"]:
            out[k] = "identical"
        elif a[k]["ops"] == b[k]["ops"] and a[k]["hsa"] == b[k]["hsa"] and a[k]["meta"] == b[k]["meta"]:
            out[k] = "equivalent"
        else:
            out[k] = "DIFFERENT"
    return out


def makefile_flags(tree):
    text = open(os.path.join(tree, CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*:=\s*(.*)$", text, re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", text, re.M).group(1)
    return hipcc, flags.replace("$(EXTRA)", "").replace("$(ARCH)", arch).split()


def compile_asm(tree, name, det, out):
    hipcc, flags = makefile_flags(tree)
    cmd = [hipcc] + flags + (["-DVS_DET_BUILD=1"] if det else []) + ["--cuda-device-only", "-S", name, "-o", out]
    r = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError("%s\n%s" % (" ".join(cmd), r.stderr[-3000:]))
    return out


def main():
    args, moved = sys.argv[1:], collections.OrderedDict()
    while "--moved" in args:
        i = args.index("--moved")
        o, ns = args[i + 1].split("=")
        moved[os.path.basename(o)] = [os.path.basename(f) for f in ns.split(",")]
        del args[i:i + 2]
    old, new = os.path.abspath(args[0]), os.path.abspath(args[1])
    taken = set(moved) | set(f for ns in moved.values() for f in ns)
    files = [os.path.basename(f) for f in args[2:]] or sorted(f for f in os.listdir(os.path.join(new, CSRC)) if f.endswith(".hip") and f not in taken)
    pairs = [(f, [f]) for f in files] + list(moved.items())         # (a file of the old tree, the files of the new tree that hold its code)
    totals, bad = collections.Counter(), 0
    with tempfile.TemporaryDirectory() as d, concurrent.futures.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        jobs = {(f, det, side): pool.submit(compile_asm, tree, f, det, os.path.join(d, "%s.%d.%s.s" % (f, det, side)))
                for o, ns in pairs for det in (0, 1) for side, tree, fs in (("old", old, [o]), ("new", new, ns)) for f in fs}
        for o, ns in pairs:
            for det in (0, 1):
                verdicts = compare_moved(open(jobs[o, det, "old"].result()).read(), [open(jobs[f, det, "new"].result()).read() for f in ns])
                names = subprocess.run(["c++filt"] + list(verdicts), capture_output=True, text=True).stdout.split("\n")
                count = collections.Counter(verdicts.values())
                print("%s %s: %s" % (o if ns == [o] else "%s -> %s" % (o, ", ".join(ns)), "VS_DET_BUILD=1" if det else "plain",
                                     ", ".join("%d %s" % (n, v) for v, n in sorted(count.items())) or "no device code"))
                for (sym, v), name in zip(verdicts.items(), names):
                    if set(count) != {"identical"}:             # a file whose every symbol is identical is its summary line
                        print("  %-12s %s" % (v, name.strip() or sym))
                totals.update(count)
                bad += sum(n for v, n in count.items() if v not in ("identical", "equivalent"))
    print("total over %d files x 2 builds: %s" % (len(pairs),", ".join("%d %s" % (n, v) for v, n in sorted(totals.items()))))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
