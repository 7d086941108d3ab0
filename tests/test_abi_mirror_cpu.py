"""matcha/_abi.py, the hand-written Python mirror of the C ABI, held to include/*.h.  No GPU, no library load.

  prototypes   every mtts_*(...) prototype is parsed from the headers and each parameter / return type classified by
               its C text; _abi.SIGNATURES must list exactly those names with the same kind at every position
  layout       one C probe including the five headers is built with the host compiler and run: sizeof / offsetof /
               member size of every _abi struct and the value of every MTTS_* constant must equal ctypes'; the
               typedefs' member names, in order, must equal the mirrors' _fields_
  coverage     every object-like integer macro of the headers is in _abi or in NOT_MIRRORED below
"""
from __future__ import annotations

import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from matcha import _abi
from test_native_abi import declared_symbols

INCLUDE = Path(__file__).resolve().parent.parent / "include"
HEADERS = sorted(INCLUDE.glob("*.h"))

# (macro, one-word reason): integer macros of the headers that Python never passes or compares
NOT_MIRRORED: tuple = ()


def _text() -> str:
    """The five headers, comments removed."""
    return re.sub(r"/\*.*?\*/", " ", "\n".join(h.read_text() for h in HEADERS), flags=re.S)


# ------------------------------------------------------------------------------------------------ prototypes
_SCALARS = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "uint32_t": "u32", "float": "f32", "double": "f64",
            "size_t": "size", "void": "void"}


def c_kind(decl: str) -> str:
    """Kind of a C parameter or return type from its text (`const float *x`, `int32_t out[6]`, `size_t`)."""
    if "*" in decl or "[" in decl:
        return "ptr"
    words = [w for w in decl.split() if w != "const"]  # `type` or `type name`
    if len(words) not in (1, 2) or words[0] not in _SCALARS:
        raise ValueError(f"unreadable C type: {decl!r}")
    return _SCALARS[words[0]]


def ctypes_kind(t) -> str:
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "ptr"
    return {ctypes.c_int32: "i32", ctypes.c_int64: "i64", ctypes.c_uint32: "u32", ctypes.c_float: "f32",
            ctypes.c_double: "f64", ctypes.c_size_t: "size"}[t]  # c_int is c_int32 here


def parse_prototypes(text: str) -> dict:
    """name -> (return kind, [parameter kinds]) for every `type mtts_name(params);` of the headers."""
    protos = {}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)  # a #define's line is no part of the next return type
    for m in re.finditer(r"([A-Za-z_][\w \t\n\*]*?)\b(mtts_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        assert name not in protos, f"{name} declared twice"
        args = [] if params in ("", "void") else [c_kind(p) for p in params.split(",")]
        protos[name] = (c_kind(ret), args)
    return protos


def signature_mismatches(protos: dict, signatures: dict) -> list[str]:
    bad = [f"{n}: in the headers, not in SIGNATURES" for n in sorted(set(protos) - set(signatures))]
    bad += [f"{n}: in SIGNATURES, not in the headers" for n in sorted(set(signatures) - set(protos))]
    for n in sorted(set(protos) & set(signatures)):
        want = protos[n]
        got = ctypes_kind(signatures[n][0]), [ctypes_kind(a) for a in signatures[n][1]]
        if want[0] != got[0]:
            bad.append(f"{n}: returns {want[0]}, mirrored as {got[0]}")
        if len(want[1]) != len(got[1]):
            bad.append(f"{n}: {len(want[1])} parameters, mirrored with {len(got[1])}")
        else:
            bad += [f"{n}: parameter {i} is {w}, mirrored as {g}"
                    for i, (w, g) in enumerate(zip(want[1], got[1])) if w != g]
    return bad


def test_every_prototype_is_parsed():
    protos = parse_prototypes(_text())
    syms = declared_symbols()
    assert len(syms) == 85
    assert sorted(protos) == syms  # a prototype the parser cannot read fails here rather than vanish


def test_signatures_match_the_prototypes():
    assert not signature_mismatches(parse_prototypes(_text()), _abi.SIGNATURES)


def test_a_swapped_int_and_pointer_is_reported():
    name = "mtts_mel_from_wav"  # (const void *wav, int32_t wav_is_int16, ...)
    restype, argtypes = _abi.SIGNATURES[name]
    swapped = [argtypes[1], argtypes[0], *argtypes[2:]]
    assert ctypes_kind(swapped[0]) == "i32" and ctypes_kind(swapped[1]) == "ptr"
    bad = signature_mismatches(parse_prototypes(_text()), {**_abi.SIGNATURES, name: (restype, swapped)})
    assert bad == [f"{name}: parameter 0 is ptr, mirrored as i32", f"{name}: parameter 1 is i32, mirrored as ptr"]


# ---------------------------------------------------------------------------------- struct layout, macro values
def mirrors() -> list:
    return [v for v in vars(_abi).values() if hasattr(v, "_c_name_")]


def constants() -> dict:
    return {k: v for k, v in vars(_abi).items() if k.startswith("MTTS_") and isinstance(v, int)}


def parse_typedefs(text: str) -> dict:
    """C struct name -> member names in order, for every `typedef struct ... { ... } mtts_x;` of the headers."""
    out = {}
    for m in re.finditer(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(mtts_\w+)\s*;", text):
        names = []
        for decl in m.group(1).split(";"):
            if decl.strip():
                first, *rest = decl.split(",")  # `const float *q, *k, *v` / `int32_t off[MTTS_CONV_MAX_TAPS]`
                for d in [first, *rest]:
                    names.append(re.findall(r"[A-Za-z_]\w*", d.split("[")[0])[-1])
        out[m.group(2)] = names
    return out


def _compiler() -> str | None:
    for cand in (os.environ.get("CC"), "cc", "gcc", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang"):
        path = shutil.which(cand) if cand else None
        if path:
            return path
    return None


def layout_mismatches(measured: dict, structs: list, consts: dict) -> list[str]:
    """measured: the probe's `key value` lines; compared with ctypes' view of the mirrors."""
    bad = []
    for s in structs:
        c = s._c_name_
        if measured[f"sizeof {c}"] != ctypes.sizeof(s):
            bad.append(f"{c}: sizeof {measured[f'sizeof {c}']}, mirrored as {ctypes.sizeof(s)}")
        for name, _ in s._fields_:
            f = getattr(s, name)
            want = (measured[f"offsetof {c} {name}"], measured[f"sizeof {c} {name}"])
            if want != (f.offset, f.size):
                bad.append(f"{c}.{name}: (offset, size) {want}, mirrored as {(f.offset, f.size)}")
    bad += [f"{k}: {measured[f'value {k}']}, mirrored as {v}" for k, v in consts.items() if measured[f"value {k}"] != v]
    return bad


@pytest.fixture(scope="module")
def measured(tmp_path_factory) -> dict:
    cc = _compiler()
    if cc is None:
        pytest.skip("no host C compiler ($CC, cc, gcc, ROCm's clang)")
    lines = ["#include <stdio.h>", *[f'#include "{h.name}"' for h in HEADERS], "int main(void) {"]
    for s in mirrors():
        c = s._c_name_
        lines.append(f'printf("sizeof {c} %zu\\n", sizeof({c}));')
        for name, _ in s._fields_:
            lines.append(f'printf("offsetof {c} {name} %zu\\n", offsetof({c}, {name}));')
            lines.append(f'printf("sizeof {c} {name} %zu\\n", sizeof((({c} *)0)->{name}));')
    lines += [f'printf("value {k} %lld\\n", (long long)({k}));' for k in constants()]
    lines += ["return 0;", "}"]
    tmp = tmp_path_factory.mktemp("abi_probe")
    (tmp / "probe.c").write_text("\n".join(lines) + "\n")
    subprocess.run([cc, f"-I{INCLUDE}", "-o", str(tmp / "probe"), str(tmp / "probe.c")], check=True)
    out = subprocess.run([str(tmp / "probe")], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.splitlines())}


def test_struct_layouts_and_constants_match_the_compiler(measured):
    assert measured["sizeof mtts_conv_gemm_args"] == 208 and measured["sizeof mtts_pack_job"] == 80  # the probe ran
    assert not layout_mismatches(measured, mirrors(), constants())


def test_two_exchanged_fields_are_reported(measured):
    grad, offset, n, pad = _abi.AdamWChunk._fields_

    class Swapped(_abi.AdamWChunk.__base__):  # a structure like mtts_adamw_chunk's mirror, `offset` and `n` exchanged
        _c_name_ = "mtts_adamw_chunk"
        _fields_ = [grad, n, offset, pad]

    bad = layout_mismatches(measured, [Swapped], {})
    assert any(b.startswith("mtts_adamw_chunk.n:") for b in bad) and any(".offset:" in b for b in bad), bad
    assert [n for n, _ in Swapped._fields_] != parse_typedefs(_text())["mtts_adamw_chunk"]


def test_every_typedef_has_a_mirror_with_its_member_names():
    typedefs = parse_typedefs(_text())
    by_name = {s._c_name_: s for s in mirrors()}
    assert len(by_name) == len(mirrors())
    assert set(typedefs) == set(by_name)
    for c, names in typedefs.items():
        assert [n for n, _ in by_name[c]._fields_] == names, c


# -------------------------------------------------------------------------------------------- macro coverage
def test_every_integer_macro_is_mirrored_or_listed():
    macros = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MTTS_[A-Z0-9_]+)[ \t]+([^\n]*\S)", _text(), flags=re.M)
    ints = [n for n, body in macros if re.fullmatch(r"[0-9a-fA-FxXlLuU \t()<|+*-]+", body)]
    assert len(ints) == len(macros) >= 40, [n for n, _ in macros if n not in ints]  # every one is an integer
    listed = [n for n, _reason in NOT_MIRRORED]
    consts = constants()
    assert not [n for n in ints if n not in consts and n not in listed]
    assert not [n for n in listed if n in consts or n not in ints]  # nothing listed that is mirrored or gone
