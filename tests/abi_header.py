"""include/real_hip.h read as text -- TEST INFRASTRUCTURE ONLY: the members of every struct it declares, for the tests that hold
real_amd/lib.py against it (test_mirror_cpu.py checks all of them; the per-feature abi tests name the ones they add)."""
import ctypes as C
import os
import re

from real_amd import lib as rlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_structs() -> dict:
    """{name: [member names in order]} of every `typedef struct real_hip_X { ... } real_hip_X;` of the header: comments are
    dropped, `a, b` declares two members, `x[4]` and `*p` declare x and p"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "real_hip.h")).read(), flags=re.S)
    out = {}
    for name, body in re.findall(r"typedef struct (real_hip_\w+) \{(.*?)\} \1;", hdr, re.S):
        names = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            kind, rest = re.fullmatch(r"((?:const\s+)?\w+)\b(.*)", decl, re.S).groups()
            names += [re.sub(r"\[\w+\]|[*\s]", "", n) for n in rest.split(",")]
        assert names and all(re.fullmatch(r"[A-Za-z_]\w*", n) for n in names), (name, names)
        out[name] = names
    return out


def mirror_of(name: str):
    """the ctypes.Structure of lib.py for a struct of the header (real_hip_pair_all_stats -> RealHipPairAllStats), or None"""
    cls = getattr(rlib, "".join(w.capitalize() for w in name.split("_")), None)
    return cls if isinstance(cls, type) and issubclass(cls, C.Structure) else None
