"""The C-ABI library loads and exports exactly the symbols include/loner_amd.h declares; the binding
loner_amd/_lib.py reads from that header agrees with the C compiler and refuses what it does not know;
host-only entry points agree with the oracle.  CPU only (no kernel launches)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import hashgrid as ohg
from oracle import rng as orng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "loner_amd.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(lnr_\w+)\s*\(", src)))


def _tool(*names):
    """The first of ``names`` on PATH or in the ROCm tree's LLVM, or None."""
    from loner_amd import build as B
    llvm = os.path.join(os.path.dirname(os.path.dirname(B.HIPCC)), "llvm", "bin")
    return next((t for n in names for t in (shutil.which(n), shutil.which(n, path=llvm)) if t), None)


@pytest.fixture(scope="module")
def L():
    from loner_amd import _lib
    return _lib


def test_library_exports_header(L):
    lib = L.lib()
    declared = _declared()
    assert len(declared) >= 25
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/loner_amd.h but not exported"
    assert set(declared) == set(L.exported_symbols()), set(declared) ^ set(L.exported_symbols())
    assert lib.lnr_version() == 1
    # the reverse: the library exports nothing the header does not declare (loner_amd/build.py's promise)
    nm = _tool("llvm-nm", "nm")
    if nm is None:
        pytest.skip("no nm to list the library's dynamic symbols")
    out = subprocess.run([nm, "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    exported = {n for n in exported if n.startswith("lnr_") and not n.startswith("lnr_debug_phases_")}
    assert len(exported) >= 25
    assert exported <= set(declared), f"exported but not in include/loner_amd.h: {sorted(exported - set(declared))}"


_C_NAMES = {ctypes.c_int32: "int32_t", ctypes.c_uint32: "uint32_t", ctypes.c_int64: "int64_t", ctypes.c_float: "float",
            ctypes.c_double: "double"}


def _c_check_source(header):
    """C text that compiles next to the real header only if ``header`` (a parsed one) states the same ABI: every
    function declared again from its parsed pieces, every struct's size, field offsets, element types and lengths."""
    c_names = {**_C_NAMES, **{cls: name for name, cls in header.structs.items()}}
    out = ["#include <stddef.h>", '#include "loner_amd.h"']
    for name, f in header.functions.items():
        out.append(f"{f.ret} {name}({', '.join(f'{t} {n}' for t, n in f.params) or 'void'});")
    for name, cls in header.structs.items():
        out.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(cls)}, "sizeof {name}");')
        for field, t in cls._fields_:
            what, member = f'"{name}.{field}"', f"(({name}*)0)->{field}"
            out.append(f"_Static_assert(offsetof({name}, {field}) == {getattr(cls, field).offset}, {what});")
            if issubclass(t, ctypes.Array):
                out.append(f"_Static_assert(sizeof({member}) / sizeof({member}[0]) == {t._length_}, {what});")
                t, member = t._type_, member + "[0]"
            if t is ctypes.c_void_p:
                out.append(f"_Static_assert(sizeof({member}) == sizeof(void*), {what});")
            else:
                out.append(f"_Static_assert(_Generic({member}, {c_names[t]}: 1, default: 0), {what});")
    return "\n".join(out) + "\n"


def _compile_check(header, tmp_path):
    cc = _tool("cc", "gcc", "clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "abi_check.c"
    src.write_text(_c_check_source(header))
    return subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", INCLUDE, str(src)], capture_output=True, text=True)


def test_binding_agrees_with_the_c_compiler(L, tmp_path):
    header = L.parse_header()
    assert (len(header.functions), len(header.structs)) == (len(L.FUNCTIONS), len(L.STRUCTS))
    assert len(header.functions) >= 80 and len(header.structs) >= 11
    r = _compile_check(header, tmp_path)
    assert r.returncode == 0, r.stderr


def test_swapped_parameters_do_not_compile(L, tmp_path):
    text = open(HEADER).read()
    swapped = re.sub(r"(int32_t n_kf)(,\s*)(int64_t step)(, double lr)", r"\3\2\1\4", text)
    assert swapped != text
    (tmp_path / "swapped.h").write_text(swapped)
    header = L.parse_header(str(tmp_path / "swapped.h"))
    assert [t for t, _ in header.functions["lnr_pose_adam"].params][5:7] == ["int64_t", "int32_t"]
    r = _compile_check(header, tmp_path)
    assert r.returncode != 0 and "conflicting types" in r.stderr and "lnr_pose_adam" in r.stderr, r.stderr


_GOOD = ("#define LNR_N (1 << 2)\ntypedef struct lnr_a {\n  float x[LNR_N + 1], *p;\n} lnr_a;\n"
         "int lnr_f(const lnr_a* a);\n")
_REFUSED = {  # what the parser must refuse: (text after _GOOD, the 1-based line it must name)
    "bit-field": ("typedef struct lnr_b {\n  int32_t x;\n  uint32_t flags : 3;\n} lnr_b;\n", 8),
    "union in a struct": ("typedef struct lnr_b {\n  int32_t x;\n  union { int32_t i; float f; } u;\n} lnr_b;\n", 8),
    "union": ("int lnr_g(void);\ntypedef union lnr_u { int32_t i; float f; } lnr_u;\n", 7),
    "function-pointer parameter": ("int lnr_g(int32_t n,\n          void (*done)(int32_t), void* stream);\n", 6),
    "unknown scalar parameter": ("int lnr_g(const float* x,\n          size_t n);\n", 7),
    "unknown scalar field": ("typedef struct lnr_b {\n  size_t n;\n} lnr_b;\n", 7),
    "function-like macro": ("#define LNR_SQ(x) ((x) * (x))\n", 6),
    "identifier outside the whitelist": ("#define LNR_OK 0\n#define LNR_BYTES (sizeof(float) * LNR_N)\n", 7),
    "operator outside the whitelist": ("#define LNR_HALF (LNR_N / 2)\n", 6),
    "later name": ("#define LNR_A LNR_B\n#define LNR_B 1\n", 6),
    "unterminated prototype": ("int lnr_g(void);\nint lnr_h(int32_t n, void* stream)\nint lnr_i(void);\n", 7),
    "prototype cut off": ("int lnr_g(int32_t n,\n", 6),
    "unnamed parameter": ("int lnr_g(int32_t, void* stream);\n", 6),
}


def test_parser_reads_its_forms(L, tmp_path):
    (tmp_path / "good.h").write_text(_GOOD)
    h = L.parse_header(str(tmp_path / "good.h"))
    a = h.structs["lnr_a"]
    assert h.constants == {"N": 4} and list(h.functions) == ["lnr_f"]
    assert [(n, ctypes.sizeof(t)) for n, t in a._fields_] == [("x", 20), ("p", 8)] and a.p.offset == 24
    assert h.functions["lnr_f"].params == [("const lnr_a*", "a")] and h.functions["lnr_f"].argtypes == [ctypes.c_void_p]
    with pytest.raises(RuntimeError, match="not found"):
        L.parse_header(str(tmp_path / "absent.h"))


@pytest.mark.parametrize("case", list(_REFUSED))
def test_parser_refuses_what_it_does_not_know(L, tmp_path, case):
    text, line = _REFUSED[case]
    path = tmp_path / "bad.h"
    path.write_text(_GOOD + text)
    with pytest.raises(RuntimeError) as e:
        L.parse_header(str(path))
    shown = (_GOOD + text).splitlines()[line - 1].strip()
    assert f"bad.h:{line}:" in str(e.value) and repr(shown) in str(e.value), str(e.value)


def test_call_names_the_refused_argument(L):
    with pytest.raises(ctypes.ArgumentError, match=r"lnr_sgd_step: argument 3 \(int64_t n\): "):
        L.call("lnr_sgd_step", None, None, "many", 0.1, None)
    with pytest.raises(ctypes.ArgumentError, match=r"lnr_loss_finalize: argument 3 \(const lnr_loss_params\* lp\): "):
        L.call("lnr_loss_finalize", None, 0, L.LossParams(), None, None)


def test_grid_desc_matches_tcnn_layout(L):
    for log2 in (18, 19):
        d = L.grid_desc(16, 2, log2, 16, 2.0)
        o = ohg.GridLayout(16, 2, log2, 16)
        assert d.n_entries == o.n_entries
        assert list(d.size[:16]) == o.sizes
        assert list(d.offset[:16]) == o.offsets
        assert list(d.resolution[:16]) == o.resolutions
        np.testing.assert_array_equal(np.array(d.scale[:16], np.float32), np.array(o.scales, np.float32))


def test_step_key_matches_oracle(L):
    for seed, step in [(0, 0), (1, 7), (123456, 99999)]:
        assert L.step_key(seed, step) == orng.step_key(seed, step)


def test_error_contract(L):
    d = L.GridDesc()
    rc = L.lib().lnr_grid_desc_init(ctypes.byref(d), 16, 3, 18, 16, 2.0)
    assert rc == -1
    assert b"n_features_per_level=2" in L.lib().lnr_last_error()
    with pytest.raises(RuntimeError, match="n_levels"):
        L.grid_desc(0, 2, 18, 16)
