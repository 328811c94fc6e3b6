#!/usr/bin/env python3
"""Record the import surface that the reference's hot-path modules take from `gsplat`, `bilateral` and `nvdiffrast`.

    python oracle/gen_golden_reference_imports.py <reference project directory>

Parses (``ast``, nothing is executed) models/gaussians/basics.py, models/gaussians/vanilla.py and models/modules.py of the
reference project and writes every ``from <pkg>... import <names>`` and ``import <pkg>... as <alias>`` of those three packages --
with the attributes each alias is used for -- to tests/golden/reference_dropin_imports.json.  The fixture holds module and name
strings only; tests/test_abi_and_host.py resolves them against this repository's drop-in packages (bilateral_driving_amd/dropin).
"""
import ast
import json
import os
import sys

MODULES = ("models/gaussians/basics.py", "models/gaussians/vanilla.py", "models/modules.py")
PACKAGES = ("gsplat", "bilateral", "nvdiffrast")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "reference_dropin_imports.json")


def surface(path: str, rel: str) -> list:
    tree = ast.parse(open(path).read(), filename=rel)
    out, aliases = [], {}
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] in PACKAGES:
            out.append({"file": rel, "line": node.lineno, "module": node.module, "names": [a.name for a in node.names]})
        elif isinstance(node, ast.Import):
            for a in node.names:
                if a.name.split(".")[0] in PACKAGES:
                    entry = {"file": rel, "line": node.lineno, "module": a.name, "alias": a.asname or a.name, "attributes": []}
                    aliases[entry["alias"]] = entry
                    out.append(entry)
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id in aliases:
            attrs = aliases[node.value.id]["attributes"]
            if node.attr not in attrs:
                attrs.append(node.attr)
    for entry in aliases.values():
        entry["attributes"].sort()
    return sorted(out, key=lambda e: e["line"])


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    root = sys.argv[1]
    imports = []
    for rel in MODULES:
        imports += surface(os.path.join(root, rel), rel)
    assert imports, f"no imports of {PACKAGES} found under {root}"
    with open(OUT, "w") as f:
        json.dump({"modules": list(MODULES), "packages": list(PACKAGES), "imports": imports}, f, indent=1)
        f.write("\n")
    print(f"{len(imports)} import statements -> {os.path.normpath(OUT)}")


if __name__ == "__main__":
    main()
