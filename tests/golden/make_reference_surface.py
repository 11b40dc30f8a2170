"""Generates tests/golden/reference_surface.json: the drop-in boundary of the reference package as data.

test_reference_surface.py pins this package's extension and Python surface against the reference's.  The reference checkout is
not part of this repository and is not present where the suite runs, so what those tests need of it is recorded here once: the
names its Python imports from `torch_bnb_fp4_ext`, the arity of every call to them, the parameter types of the functions its C++
binds, and the parameter names and defaults of its public Python functions and methods.  The reference is PARSED (never imported),
and only these facts are written - no source text.  Run from the repo root with the path of a reference checkout:

    python tests/golden/make_reference_surface.py <reference checkout>
"""
import ast
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_surface.json")


def ext_imports(tree):
    """{local alias: extension attribute} for every `from torch_bnb_fp4_ext import X as Y`."""
    out = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.module == "torch_bnb_fp4_ext":
            for a in node.names:
                out[a.asname or a.name] = a.name
        elif isinstance(node, ast.Import):
            assert all(a.name != "torch_bnb_fp4_ext" for a in node.names), "module-style import: extend this generator"
    return out


def ext_call_sites(tree, imports):
    """Every call of an imported extension function (ScalarType aside): line, positional / keyword argument counts, *args."""
    calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id in imports
             and imports[n.func.id] != "ScalarType"]
    return sorted(({"function": imports[c.func.id], "line": c.lineno, "positional_args": len(c.args), "keyword_args": len(c.keywords),
                    "starred": any(isinstance(a, ast.Starred) for a in c.args)} for c in calls), key=lambda r: r["line"])


def scalar_type_members(tree):
    return sorted({n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == "ScalarType_"})


def _params(fn: ast.FunctionDef):
    a = fn.args
    names = [x.arg for x in a.posonlyargs + a.args if x.arg not in ("self", "cls")]
    pos = [x.arg for x in a.posonlyargs + a.args]
    defaults = {}
    for name, d in zip(pos[len(pos) - len(a.defaults):], a.defaults):
        try:
            value = ast.literal_eval(d)
            # (JSON gives lists back as lists; a tuple would come back as a list and compare unequal)
            assert json.loads(json.dumps(value)) == value, f"{fn.name}({name}=...): extend the JSON encoding for {value!r}"
            defaults[name] = {"literal": value}
        except (ValueError, SyntaxError):
            defaults[name] = {"expression": ast.unparse(d)}  # torch.float16, torch.device(...): compared as text by the test
    return names, defaults


def python_surface(tree):
    """Module-level functions and the methods of every module-level class, in source order."""
    out = []
    for node in tree.body:
        if isinstance(node, ast.FunctionDef):
            names, defaults = _params(node)
            out.append({"class": None, "name": node.name, "params": names, "defaults": defaults})
        elif isinstance(node, ast.ClassDef):
            out.append({"class": node.name, "name": None, "params": None, "defaults": None})
            for m in node.body:
                if isinstance(m, ast.FunctionDef):
                    names, defaults = _params(m)
                    out.append({"class": node.name, "name": m.name, "params": names, "defaults": defaults})
    return out


def cpp_bindings(text):
    """{python name: [C++ parameter types]} from PYBIND11_MODULE's m.def lines and the definitions they point at, and the enum's values."""
    text = re.sub(r"//[^\n]*", "", text)
    defs = dict(re.findall(r'm\.def\(\s*"(\w+)"\s*,\s*&(\w+)', text))
    enum_values = re.findall(r'\.value\(\s*"(\w+)"', text)
    out = {}
    for py_name, cpp_name in defs.items():
        m = re.search(r"torch::Tensor\s+" + cpp_name + r"\s*\(([^)]*)\)\s*\{", text)
        assert m, cpp_name
        params = [p.strip() for p in m.group(1).split(",") if p.strip()]
        out[py_name] = [p.rsplit(None, 1)[0].replace("const ", "").replace("&", "").strip() for p in params]
    return out, sorted(enum_values)


def main(ref_root):
    tree = ast.parse(open(os.path.join(ref_root, "torch_bnb_fp4", "__init__.py")).read())
    imports = ext_imports(tree)
    bindings, enum_values = cpp_bindings(open(os.path.join(ref_root, "csrc", "torch_fp4.cpp")).read())
    rec = {
        "_what": "the reference package's drop-in boundary, parsed from its torch_bnb_fp4/__init__.py and csrc/torch_fp4.cpp "
                 "(tests/golden/make_reference_surface.py); line numbers are the reference's",
        "ext_imports": imports,
        "scalar_type_members": scalar_type_members(tree),
        "ext_call_sites": ext_call_sites(tree, imports),
        "cpp_bindings": bindings,
        "cpp_enum_values": enum_values,
        "python_surface": python_surface(tree),
    }
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", os.path.relpath(OUT), f"({len(rec['python_surface'])} surface entries, {len(rec['ext_call_sites'])} call sites)")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(f"usage: python {sys.argv[0]} <reference checkout>")
    main(sys.argv[1])
