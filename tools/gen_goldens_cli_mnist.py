#!/usr/bin/env python
"""Generate tests/golden/cli_flags_mnist.json: the command-line flags of the reference's MNIST+FashionMNIST scripts and of its
GOLD-only phase-2 scripts (development machine only).

    python tools/gen_goldens_cli_mnist.py --reference <checkout of the reference>

The scripts are READ, not imported (importing them needs torch_mimicry): every `parser.add_argument(...)` call is taken from
the syntax tree and its literal arguments are evaluated.  The file holds data only -- per script the list of
[option strings, default, kind] with kind the name of `type=` ('str', 'int', 'float') or of `action=` ('store_true') -- and
nothing of the scripts' text.  tests/test_pacgan_host.py compares diagan/cli.py's tables with it.
"""
import argparse
import ast
import json
import os

SCRIPTS = ("train_mimicry_mnist_fmnist_phase1.py", "train_mimicry_mnist_fmnist_phase2.py",
           "train_mimicry_color_mnist_phase2_gold.py", "train_mimicry_mnist_fmnist_phase2_gold.py")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def flags_of(path):
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    rows = []
    for node in ast.walk(tree):
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument"):
            continue
        names = [ast.literal_eval(a) for a in node.args]
        kw = {k.arg: k.value for k in node.keywords}
        if "action" in kw:
            kind, default = ast.literal_eval(kw["action"]), False
            if kind != "store_true":
                raise ValueError(f"{path}:{node.lineno}: action {kind!r} is not one the tables of diagan/cli.py know")
        else:
            kind = kw["type"].id if "type" in kw else "str"
            default = ast.literal_eval(kw["default"]) if "default" in kw else None
        dest = ast.literal_eval(kw["dest"]) if "dest" in kw else None
        if dest is not None and dest != names[0].lstrip("-"):
            raise ValueError(f"{path}:{node.lineno}: dest {dest!r} differs from the option's own name")
        rows.append((node.lineno, [names, default, kind]))
    return [row for _, row in sorted(rows, key=lambda r: r[0])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory that holds the reference's train_mimicry_*.py scripts")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "cli_flags_mnist.json"))
    args = ap.parse_args()
    table = {name: flags_of(os.path.join(args.reference, name)) for name in SCRIPTS}
    with open(args.out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}: " + ", ".join(f"{k} {len(v)} flags" for k, v in table.items()))


if __name__ == "__main__":
    main()
