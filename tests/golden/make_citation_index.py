#!/usr/bin/env python3
"""Generates tests/golden/reference_citations.json.

tests/test_citations_cpu.py checks the `file:line` citations of the reference (jlogan03/interpn v0.8.2) that the
oracle, the C ABI header and the kernels carry.  It needs only facts ABOUT the reference's text files, not the text:
  files          every .rs / .py / .pyi / .toml file of the reference tree (relative path, as `glob("**")` finds it)
                 with its number of lines,
  mul_add_lines  for each of those files, the 1-based numbers of the lines that contain `mul_add`.
Frozen here so that the check runs wherever the repository does.  Run from the repository root with the reference
tree's location:  python tests/golden/make_citation_index.py PATH_TO_REFERENCE
"""
import glob
import json
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_citations.json")
EXTS = (".rs", ".py", ".pyi", ".toml")


def index(ref):
    files = {}
    for p in sorted(glob.glob(os.path.join(ref, "**", "*"), recursive=True)):
        if not os.path.isfile(p) or not p.endswith(EXTS):
            continue
        rel = os.path.relpath(p, ref)
        with open(p, errors="replace") as f:
            n = sum(1 for _ in f)
        with open(p, errors="replace") as f:
            hits = [i + 1 for i, line in enumerate(f.read().split("\n")) if "mul_add" in line]
        files[rel] = {"lines": n, "mul_add_lines": hits}
    return files


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "src")):
        raise SystemExit("usage: make_citation_index.py PATH_TO_REFERENCE (the tree that holds src/)")
    rec = {"reference": "jlogan03/interpn v0.8.2", "files": index(sys.argv[1])}
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{OUT}: {len(rec['files'])} files")


if __name__ == "__main__":
    main()
