"""The ctypes signature table (tskd_amd/ops/hip.py) agrees with the
``extern "C"`` prototypes of the three .hip files. Reads files and the
table only: no library is loaded and no GPU is needed."""

import ctypes
import os
import re

import pytest

from tskd_amd.ops import build, hip

CTYPE = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float,
         "unsigned long long": ctypes.c_ulonglong}
_DEF = re.compile(r"^int\s+(tskd_\w+)\s*\(([^)]*)\)\s*\{", re.M)


def _param_ctype(param):
    if "*" in param:
        return ctypes.c_void_p
    words = param.replace("const", " ").split()
    ctype = " ".join(words[:-1])  # the last word is the parameter's name
    assert ctype in CTYPE, f"parameter type outside the mapping: {param!r}"
    return CTYPE[ctype]


def _exported(lib):
    """{function name: argtypes} parsed from the library's extern "C" block."""
    (src,) = build.SOURCES[lib]
    with open(os.path.join(build.CSRC, src), encoding="utf-8") as fh:
        text = fh.read()
    block = text.split('extern "C" {', 1)[1].split('}  // extern "C"', 1)[0]
    # every exported definition is caught: nothing named tskd_* is missed
    assert len(_DEF.findall(block)) == len(
        re.findall(r"^\w[\w \t]*\btskd_\w+\s*\(", block, re.M))
    return {name: [_param_ctype(p.strip()) for p in params.split(",")]
            for name, params in _DEF.findall(block)}


@pytest.mark.parametrize("lib", sorted(hip.SIGNATURES))
def test_table_matches_prototypes(lib):
    exported = _exported(lib)
    assert exported, f"no extern \"C\" definitions found for {lib}"
    table = hip.SIGNATURES[lib]
    assert not set(table) - set(exported), "table names unexported functions"
    assert not set(table) & hip.UNBOUND
    for name, argtypes in exported.items():
        if name in table:
            assert table[name] == argtypes, name
        else:
            assert name in hip.UNBOUND, f"{name} is exported but not bound"


def test_every_library_and_unbound_name_is_real():
    assert set(hip.SIGNATURES) == set(build.SOURCES)
    exported = set().union(*(_exported(lib) for lib in hip.SIGNATURES))
    assert hip.UNBOUND <= exported
    assert sum(len(_exported(lib)) for lib in hip.SIGNATURES) == \
        sum(len(t) for t in hip.SIGNATURES.values()) + len(hip.UNBOUND)
