"""ctypes binding of the C ABI in ``include/loner_amd.h`` (``loner_amd/_lib/libloner_amd.so``).

The library is built in-tree by ``python -m loner_amd.build`` (or ``__graft_entry__.build()``).
There is no fallback: if the library is missing or a call fails, a RuntimeError is raised —
mirroring tiny-cuda-nn's ``CHECK_THROW`` behaviour at the same boundary.

The binding is read from the header at import (``parse_header``); nothing of the ABI is restated here.
  - ``#define LNR_X <expr>`` becomes the module constant ``X``.  ``<expr>`` holds integer and float literals
    (``u`` suffix allowed), ``INT64_MAX``, earlier ``LNR_`` names and ``+ - * << ( )``, nothing else.
    ``LOSS_KINDS``, ``RENDER_STRATEGIES`` and ``SELECT`` are the ``LNR_LOSS_*``, ``LNR_RENDER_*`` and ``LNR_SELECT_*``
    groups.
  - ``typedef struct lnr_x {...} lnr_x;`` becomes a ``ctypes.Structure`` (``lnr_grid_desc`` -> ``GridDesc``): the
    fields in order, fixed-width scalars by ``_SCALARS``, ``name[expr]`` an array, an earlier ``lnr_`` struct by value.
  - ``ret lnr_name(params);`` gives the function's restype and argtypes (``FUNCTIONS``); ``int`` is also a scalar here.
  - Every pointer is ``c_void_p`` (device tensors, ``byref(struct)`` and struct arrays in device memory all pass
    through it); a ``const char*`` return is ``c_char_p``.
  - A line that fits none of these is an error naming the line, never skipped.

torch is imported before the library is loaded so that the library binds to the HIP runtime
torch already loaded (one runtime per process; streams are shared).
"""
import collections
import ctypes
import os
import re

import torch  # noqa: F401  (must precede the dlopen, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libloner_amd.so")
# Kernel experiments load an alternative in-tree build (tools/exp_variants.py); unset in production.
LIB_PATH = os.environ.get("LONER_AMD_LIB", LIB_PATH)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "loner_amd.h")

_SCALARS = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
            "float": ctypes.c_float, "double": ctypes.c_double}
_PROTO_SCALARS = dict(_SCALARS, int=ctypes.c_int)
_CLASS_NAMES = {"lnr_ray_window": "RayWindowDesc"}  # loner_amd.rays.RayWindow is the class that fills it

Header = collections.namedtuple("Header", "constants structs functions")
# ret and params hold the C spelling: "const char*", [("const lnr_loss_params*", "lp"), ...]
Function = collections.namedtuple("Function", "restype argtypes ret params")

_TOKEN = re.compile(r"\s*(?:(0[xX][0-9a-fA-F]+|\d+(?:\.\d*)?(?:[eE][-+]?\d+)?)[uU]?|(LNR_\w+|INT64_MAX)|(<<|[-+*()]))")
_SPACE = re.compile(r"\s*")
_PREPROCESSOR = re.compile(r"#\s*(?:(?:ifndef|ifdef|endif|include)\b.*|define\s+(?!LNR_)\w+)")
_DEFINE = re.compile(r"#\s*define\s+LNR_(\w+)\s+(\S.*)")
_EXTERN_C = re.compile(r'extern\s+"C"\s*\{|\}')
_TYPE = r"((?:const\s+)?\w+)"
_STRUCT = re.compile(r"typedef\s+struct\s+(lnr_\w+)\s*\{(.*?)\}\s*(\w+)\s*;", re.S)
_FIELD = re.compile(_TYPE + r"\b(.*)", re.S)
_DECLARATOR = re.compile(r"\s*(\**)\s*(\w+)\s*(?:\[([^\[\]]+)\])?\s*")
_PROTO = re.compile(_TYPE + r"\s*(\**)\s*(lnr_\w+)\s*\(([^()]*)\)\s*;")
_PARAM = re.compile(r"\s*" + _TYPE + r"(\s*\*+\s*|\s+)(\w+)\s*")


def parse_header(path=HEADER_PATH):
    """The constants, structs and functions ``path`` declares (module docstring); RuntimeError on anything else."""
    if not os.path.exists(path):
        raise RuntimeError(f"loner_amd: C header not found ({path})")
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: "\n" * m.group().count("\n"), f.read(), flags=re.S)
    constants, structs, functions = {}, {}, {}

    def error(offset, what):
        line = text.count("\n", 0, offset) + 1
        return RuntimeError(f"{path}:{line}: {what}: {text.splitlines()[line - 1].strip()!r}")

    def evaluate(expr, offset):
        names, terms, pos = dict(constants, INT64_MAX=2 ** 63 - 1), [], 0
        while pos < len(expr.rstrip()):
            m = _TOKEN.match(expr, pos)
            if not m or (m.group(2) and m.group(2).replace("LNR_", "", 1) not in names):
                raise error(offset, f"unsupported constant expression {expr.strip()!r}")
            number, name, operator = m.groups()
            terms.append(f"({names[name.replace('LNR_', '', 1)]!r})" if name else number or operator)
            pos = m.end()
        try:
            return eval(" ".join(terms), {"__builtins__": {}})  # literals and + - * << ( ) only, checked above
        except Exception:
            raise error(offset, f"unsupported constant expression {expr.strip()!r}") from None

    def ctype(base, stars, scalars, offset, ret=False):
        if stars:
            return ctypes.c_char_p if ret and base == "const char" else ctypes.c_void_p
        if base not in scalars:
            raise error(offset, f"unknown type {base!r}")
        return scalars[base]

    def struct(m):
        name, body, alias = m.groups()
        fields = []
        for decl in re.finditer(r"[^;]*[^;\s][^;]*;", body):
            offset = m.start(2) + decl.start() + len(decl.group()) - len(decl.group().lstrip())
            f = _FIELD.fullmatch(decl.group()[:-1].strip())
            declarators = [_DECLARATOR.fullmatch(d) for d in f.group(2).split(",")] if f else [None]
            if not all(declarators):
                raise error(offset, "unrecognised struct field")
            for d in declarators:
                t = ctype(f.group(1), d.group(1), dict(_SCALARS, **structs), offset)
                fields.append((d.group(2), t * evaluate(d.group(3), offset) if d.group(3) else t))
        if alias != name or not body.rstrip().endswith(";"):
            raise error(m.start(), "unrecognised struct")
        py_name = _CLASS_NAMES.get(name) or "".join(w.capitalize() for w in name.split("_")[1:])
        structs[name] = type(py_name, (ctypes.Structure,), {"_fields_": fields})

    def prototype(m):
        base, stars, name, params = m.groups()
        restype = ctype(base, stars, _PROTO_SCALARS, m.start(), ret=True)
        argtypes, c_params = [], []
        for p in re.finditer(r"[^,]+", "" if params.strip() == "void" else params):
            offset = m.start(4) + p.start() + len(p.group()) - len(p.group().lstrip())
            pm = _PARAM.fullmatch(p.group())
            if not pm:
                raise error(offset, "unrecognised parameter")
            argtypes.append(ctype(pm.group(1), pm.group(2).strip(), _PROTO_SCALARS, offset))
            c_params.append((pm.group(1) + pm.group(2).strip(), pm.group(3)))
        if params.strip() != "void" and len(argtypes) != params.count(",") + 1:
            raise error(m.start(), "unrecognised parameter list")
        functions[name] = Function(restype, argtypes, base + stars, c_params)

    pos = 0
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos == len(text):
            break
        if text[pos] == "#":
            end = text.find("\n", pos) % (len(text) + 1)  # no newline: the text's end
            line = text[pos:end].rstrip()
            m = _DEFINE.fullmatch(line)
            if m:
                constants[m.group(1)] = evaluate(m.group(2), pos)
            elif not _PREPROCESSOR.fullmatch(line):
                raise error(pos, "unrecognised preprocessor line")
            pos = end
            continue
        for pattern, handle in ((_EXTERN_C, None), (_STRUCT, struct), (_PROTO, prototype)):
            m = pattern.match(text, pos)
            if m:
                if handle:
                    handle(m)
                pos = m.end()
                break
        else:
            raise error(pos, "unrecognised declaration")
    mentioned = re.findall(r"\b(lnr_\w+)\s*\(", re.sub(r"\{[^{}]*\}", "", text))
    if sorted(mentioned) != sorted(functions):
        raise RuntimeError(f"{path}: functions named but not parsed once each: {set(mentioned) ^ set(functions)}")
    return Header(constants, structs, functions)


_header = parse_header()
CONSTANTS, STRUCTS, FUNCTIONS = _header
globals().update(CONSTANTS)
globals().update({cls.__name__: cls for cls in STRUCTS.values()})


def _group(prefix, key=str):
    return {key(k[len(prefix):]): v for k, v in CONSTANTS.items() if k.startswith(prefix)}


LOSS_KINDS = _group("LOSS_")
RENDER_STRATEGIES = _group("RENDER_", str.lower)
SELECT = _group("SELECT_")

_lib = None


def lib():
    """Load (once) and return the ctypes library; raises RuntimeError if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"loner_amd: HIP library not built ({LIB_PATH}); run `python -m loner_amd.build`")
        L = ctypes.CDLL(LIB_PATH)
        for name, f in FUNCTIONS.items():
            fn = getattr(L, name)
            fn.restype = f.restype
            fn.argtypes = f.argtypes
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().lnr_last_error().decode(errors="replace")
        raise RuntimeError(f"{what}: {msg}" if what else msg)


def call(name, *args):
    """Call a C-ABI entry point; torch tensors are passed as device pointers.  The tensors stay
    referenced for the duration of the call; afterwards the caching allocator's stream ordering
    keeps their memory valid for the enqueued kernels."""
    conv = [ptr(a) if isinstance(a, torch.Tensor) else a for a in args]
    try:
        rc = getattr(lib(), name)(*conv)
    except ctypes.ArgumentError as e:
        raise _named(name, e) from None
    check(rc, name)
    return rc


def _named(name, e):
    """ctypes' "argument 13: TypeError: wrong type" with the function and the parameter's C declaration."""
    m = re.match(r"argument (\d+): (.*)", str(e), re.S)
    params = FUNCTIONS[name].params
    if not m or not 1 <= int(m.group(1)) <= len(params):
        return e
    c_type, c_name = params[int(m.group(1)) - 1]
    return ctypes.ArgumentError(f"{name}: argument {m.group(1)} ({c_type} {c_name}): {m.group(2)}")


def ptr(t):
    """Device pointer of a tensor (or None -> NULL).  The tensor must be contiguous and on the GPU."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("loner_amd: expected a GPU tensor (the HIP path has no CPU fallback)")
    if not t.is_contiguous():
        raise RuntimeError("loner_amd: expected a contiguous tensor")
    return ctypes.c_void_p(t.data_ptr())


def stream(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def grid_desc(n_levels=16, n_features=2, log2_hashmap_size=18, base_resolution=16, per_level_scale=2.0):
    d = GridDesc()  # noqa: F821  (lnr_grid_desc, from the header)
    check(lib().lnr_grid_desc_init(ctypes.byref(d), n_levels, n_features, log2_hashmap_size, base_resolution,
                                   per_level_scale), "lnr_grid_desc_init")
    return d


def step_key(seed, step):
    return int(lib().lnr_step_key(seed & 0xFFFFFFFF, step & 0xFFFFFFFF))


def exported_symbols():
    return sorted(FUNCTIONS)
