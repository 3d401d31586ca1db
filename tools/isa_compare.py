#!/usr/bin/env python3
"""Compare the gfx950 code of the on-demand rollout units between two trees of kernel headers.

    tools/isa_compare.py OLD_CSRC NEW_CSRC [--only TEXT] [--jobs N] [--keep DIR]

Every committed request (tests/golden/jit_records) whose template includes clik_pinv_rec.hpp or clik_qp_rec.hpp - the
recording, summarising and converging rollouts - is written out and compiled to assembly against each directory, with the
flags jit.py would use.  Per kernel: identical or not, registers / scratch / LDS / block size from the metadata, the FP64
instructions as a multiset with their encodings folded, and which lines differ next to where the loops begin.
Needs hipcc and no GPU.  Exit status 1 when a kernel differs."""
import argparse, collections, difflib, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from casclik_amd import jit  # noqa: E402

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
        ".max_flat_workgroup_size")


def units(only):
    for src, meta, _ in jit._records():
        tmpl = meta.get("template") or ""
        if "clik_pinv_rec.hpp" not in tmpl and "clik_qp_rec.hpp" not in tmpl:
            continue
        name = os.path.basename(src)[:-4]
        what = re.search(r"hipError_t (clik_jit_\w+)", tmpl).group(1)
        if only and only not in name and only not in what:
            continue
        text = meta["_text"] if "_text" in meta else open(src).read()
        yield name, what, text, meta


def assembly(csrc, path, text, meta):
    cmd = jit.unit_command(text, meta["init"], path, "-", meta.get("flags", []), meta.get("stamps", False), kind="asm",
                           csrc=csrc, sched=meta["_sched"])
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if proc.returncode != 0:
        raise RuntimeError("hipcc failed on %s against %s:\n%s" % (path, csrc, proc.stderr.decode("utf-8", "replace")[-3000:]))
    return [ln for ln in proc.stdout.decode().split("\n") if "__hip_cuid_" not in ln]


def kernels(lines):
    """{kernel: (its lines, its metadata)}"""
    out, i = {}, 0
    text = "\n".join(lines)
    info = {}
    for block in text.split("  - .agpr_count:")[1:]:
        block = "  - .agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        info[name] = tuple(int(re.search(re.escape(k) + r":\s+(\d+)", block).group(1)) for k in META)
    while i < len(lines):
        m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
        if m and m.group(1) in info:
            j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
            out[m.group(1)] = (lines[i:j], info[m.group(1)])
            i = j
        i += 1
    return out


def fp64(body):
    c = collections.Counter()
    for ln in body:
        m = re.match(r"\s+(v_\w*f64\w*)", ln)
        if m:
            c[re.sub(r"_(e32|e64|dpp|sdwa)$", "", m.group(1)).replace("v_fmac_", "v_fma_")] += 1
    return c


def loops(body):
    """line numbers of the labels that a later line branches back to"""
    at = {m.group(1): i for i, ln in enumerate(body) for m in [re.match(r"(\.LBB\d+_\d+):", ln)] if m}
    heads = set()
    for i, ln in enumerate(body):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", ln)
        if m and at.get(m.group(1), i) < i:
            heads.add(at[m.group(1)])
    return sorted(heads)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_csrc"), ap.add_argument("new_csrc")
    ap.add_argument("--only", default=""), ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 2))
    ap.add_argument("--keep", default="", help="keep the sources and both assemblies of differing units here")
    a = ap.parse_args()
    work = a.keep or tempfile.mkdtemp(prefix="isa_compare_")
    os.makedirs(work, exist_ok=True)
    todo = list(units(a.only))

    def one(u):
        name, what, text, meta = u
        path = os.path.join(work, name + ".hip")
        with open(path, "w") as f:
            f.write(text)
        return [kernels(assembly(d, path, text, meta)) for d in (a.old_csrc, a.new_csrc)]

    differ = 0
    with ThreadPoolExecutor(max_workers=a.jobs) as ex:
        for (name, what, _, _), (old, new) in zip(todo, ex.map(one, todo)):
            print("%s  %s" % (name, what))
            for k in sorted(set(old) | set(new)):
                short = re.sub(r"^_ZN4clik\d+", "", k)[:75]
                if k not in old or k not in new:
                    print("  %-75s only in %s" % (short, "OLD" if k in old else "NEW"))
                    differ += 1
                    continue
                (bo, mo), (bn, mn) = old[k], new[k]
                same, f_same = bo == bn, fp64(bo) == fp64(bn)
                differ += not same
                print("  %-75s %s  vgpr/agpr/sgpr/scratch/lds/block %s%s  fp64 %s" % (
                    short, "IDENTICAL" if same else "DIFFERS  ", "/".join(map(str, mo)),
                    "" if mo == mn else " -> " + "/".join(map(str, mn)), "equal" if f_same else "DIFFER"))
                if not f_same:
                    print("      fp64 only in old: %s, only in new: %s" % (dict(fp64(bo) - fp64(bn)), dict(fp64(bn) - fp64(bo))))
                if not same:
                    ops = [o for o in difflib.SequenceMatcher(None, bo, bn, autojunk=False).get_opcodes() if o[0] != "equal"]
                    print("      %d lines old, %d new; loops begin at old %s new %s" % (len(bo), len(bn), loops(bo), loops(bn)))
                    print("      differing old lines: %s%s" % (" ".join("%d-%d" % (o[1], o[2]) for o in ops[:24]),
                                                              " ... (%d ranges)" % len(ops) if len(ops) > 24 else ""))
                    if a.keep:
                        for tag, body in (("old", bo), ("new", bn)):
                            with open(os.path.join(work, "%s.%s.%s.s" % (name, re.sub(r"\W", "_", short), tag)), "w") as f:
                                f.write("\n".join(body))
    print("%d units, %d kernels differ" % (len(todo), differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
