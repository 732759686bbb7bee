#!/usr/bin/env python3
"""Writes ``tools_names.json``: every function / class name that the reference's four driver scripts use from its
``Tools`` package, with the ``Tools`` modules that define it.  The reference's sources are only parsed as text (``ast``),
nothing of them is stored but the names:

    python tests/golden/make_golden_names.py <directory of the reference checkout>

``tests/test_tools_dropin.py::test_every_tools_name_the_reference_drivers_use_exists`` checks the list against this
package's ``Tools``.
"""
from __future__ import annotations

import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVERS = ("Data_prepare.py", "Online_predictor.py", "Shared_extraction.py", "Model_training.py")


def names(ref):
    defined = {}
    for f in sorted(os.listdir(os.path.join(ref, "Tools"))):
        if f.endswith(".py"):
            with open(os.path.join(ref, "Tools", f)) as fh:
                for node in ast.parse(fh.read()).body:
                    if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
                        defined.setdefault(node.name, []).append(f[:-3])
    used = set()
    for drv in DRIVERS:
        with open(os.path.join(ref, drv)) as fh:
            used |= {n.id for n in ast.walk(ast.parse(fh.read())) if isinstance(n, ast.Name) and n.id in defined}
    return {name: defined[name] for name in sorted(used)}


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    out = {"drivers": list(DRIVERS), "used": names(sys.argv[1])}
    with open(os.path.join(HERE, "tools_names.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{len(out['used'])} names -> tools_names.json")


if __name__ == "__main__":
    main()
