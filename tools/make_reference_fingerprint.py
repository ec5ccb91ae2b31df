#!/usr/bin/env python3
"""tests/golden/reference_integration_fingerprint.json from a checkout of the reference (crate v0.2.4).

    python tools/make_reference_fingerprint.py <reference tree>

For every file rust/integration.patch touches: the SHA-256 of each of its lines (no text), or null when the patch creates
it; and for every `src` directory of a crate root the patch changes, the modules a `mod x;` there can name (x.rs or x/mod.rs).
It is DATA about the reference tree, enough for tests/test_rust_binding.py to check that the patch applies to it and what
the patched tree holds, without the tree."""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "reference_integration_fingerprint.json")


def line_hash(line):
    return hashlib.sha256(line.encode()).hexdigest()


def main(ref):
    patch = open(os.path.join(ROOT, "rust", "integration.patch")).read()
    files, modules = {}, {}
    for path in re.findall(r"^\+\+\+ b/(\S+)", patch, flags=re.M):
        full = os.path.join(ref, path)
        if not os.path.exists(full):
            files[path] = None
            continue
        text = open(full).read()
        files[path] = {"final_newline": text.endswith("\n"), "lines": [line_hash(l) for l in text.splitlines()]}
        src = os.path.dirname(path)
        if os.path.basename(path) in ("lib.rs", "main.rs") and os.path.basename(src) == "src":
            names = []
            for e in sorted(os.listdir(os.path.join(ref, src))):
                if e.endswith(".rs"):
                    names.append(e)
                elif os.path.isfile(os.path.join(ref, src, e, "mod.rs")):
                    names.append(e + "/mod.rs")
            modules[src] = names
    out = {"about": "reference crate v0.2.4: SHA-256 of each line of the files rust/integration.patch touches (null: the patch "
                    "creates it) and the module files of the crate roots it changes (tools/make_reference_fingerprint.py)",
           "files": files, "modules": modules}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", OUT, {k: (v and len(v["lines"])) for k, v in files.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
