#!/usr/bin/env python3
"""Per-kernel diff of two trees' device assembly (`hipcc --cuda-device-only -S` of each .hip, one .s per file).

    asm_kernel_diff.py BEFORE_DIR AFTER_DIR [-o table.json] [--rename table.json]

For every kernel symbol: identical / changed instruction text (comments, directives and local label numbers aside)
and the resource figures of both sides.  Exit status 1 if the symbol sets or any resource figure differ.  --rename: a
JSON object {symbol before: symbol after} for kernels that changed their name in between.
"""
import argparse
import json
import os
import re
import sys

FIGURES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
           ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(path):
    """-> {symbol: {"text": [instruction lines], figure: value, ...}}"""
    lines = open(path).read().splitlines()
    out, cur, labels = {}, None, {}
    for ln in lines:
        s = ln.split(";")[0].strip()
        m = re.match(r"^([A-Za-z_][\w$.]*):$", s)
        if m and not s.startswith(".L"):
            cur, labels = out.setdefault(m.group(1), {"text": []}), {}
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
        if cur is None or not s or (s.startswith(".") and not s.startswith(".L")):
            continue
        # local labels: numbered in order of first appearance inside the kernel, so that the compiler's numbering does
        # not matter and a branch to another block still does
        cur["text"].append(re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), s))
    # resource figures: amdhsa.kernels, one list entry per kernel at the outer indent, its own keys four columns in
    start = next((i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:")), len(lines))
    end = next((i for i in range(start + 1, len(lines)) if lines[i] and not lines[i].startswith(" ")), len(lines))
    for block in ("\n" + "\n".join(lines[start + 1:end])).split("\n  - ")[1:]:
        own = dict(re.findall(r"^(\.\w+): +(\S+)$", "\n".join(l[4:] for l in ("    " + block).split("\n") if l[:4] == "    "
                                                                     and l[4:5] == "."), re.M))
        if own.get(".name") in out:
            out[own[".name"]].update({f: int(own[f]) for f in FIGURES})      # (a missing figure is an error)
    return {k: v for k, v in out.items() if ".vgpr_count" in v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("-o", "--out")
    ap.add_argument("--rename")
    a = ap.parse_args()
    rename = json.load(open(a.rename)) if a.rename else {}
    was = {new: old for old, new in rename.items()}
    table, bad = [], 0
    for f in sorted(x for x in os.listdir(a.before) if x.endswith(".s")):
        kb, ka = kernels(os.path.join(a.before, f)), kernels(os.path.join(a.after, f))
        kb = {rename.get(sym, sym): k for sym, k in kb.items()}
        for sym in sorted(set(kb) | set(ka)):
            b, c = kb.get(sym), ka.get(sym)
            e = {"file": f[:-2] + ".hip", "kernel": sym}
            if sym in was:
                e["kernel_before"] = was[sym]
            if b is None or c is None:
                e["status"] = "only before" if c is None else "only after"
                bad += 1
            else:
                e["status"] = "identical" if b["text"] == c["text"] else "changed"
                e["instructions"] = [len(b["text"]), len(c["text"])]
                e["before"] = {k: b[k] for k in FIGURES}
                e["after"] = {k: c[k] for k in FIGURES}
                if e["before"] != e["after"]:
                    e["resources_differ"] = True
                    bad += 1
            table.append(e)
    for f in sorted({e["file"] for e in table}):
        rows = [e for e in table if e["file"] == f]
        print(f"{f}: {len(rows)} kernels, {sum(e['status'] == 'identical' for e in rows)} identical, "
              f"{sum(e['status'] == 'changed' for e in rows)} changed, "
              f"{sum('resources_differ' in e or e['status'].startswith('only') for e in rows)} with other figures")
        for e in rows:
            if e["status"] != "identical":
                print("   ", e["status"], e["kernel"], e.get("instructions"), "RESOURCES" if "resources_differ" in e else "")
    if a.out:
        json.dump(table, open(a.out, "w"), indent=1)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
