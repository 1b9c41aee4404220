"""ctypes binding of the C-ABI in include/gymnast_acrobot.h (libgymnast_acrobot.so), read from that header.

The header is the one statement of the ABI: its prototypes, structs, #define GYM_* constants and status codes are
parsed at import (plain re), and the argument types, struct layouts and constants bound here are what it says.  A new
entry point is its prototype in the header and its definition in a .hip file; nothing is added here.  What the
parser does not understand it refuses with an ImportError (tests/test_abi_binding_host.py checks the result against
the C compiler's reading of the header).

An extension of the ABI has a header of its own that includes the main one: every other
include/gymnast_acrobot_*.h (EXTENSION_HEADERS, from the directory, sorted; today _box.h, the torque-limited Newton
solve, _models.h, per-lane models, and _rk4lin.h, the RK4-exact linearisation).  It is read by the same parser with
the main header's structs and constants known, may declare prototypes only, and its entry points are bound beside the
others (EXTENSIONS: header -> its entry points, load()); EXPORTS, the structs and the constants stay the main
header's, and ALL_EXPORTS is EXPORTS, then each extension's entry points in EXTENSION_HEADERS' order.

ABI 18's lists are closed: the main header's prototypes, the three extension headers and each one's entry points are
what its callers and its tests know as ABI 18.  What is added to the library after them is an add-on: any other
include/*.h (ADDON_HEADERS, from the directory, sorted; today gymnast_newton_weights.h, the Newton solve on per-lane
cost weights).  An add-on is read by the same parser under the same rule as an extension (_prototypes_only: the main
header's structs and constants known, prototypes only), and load() binds its entry points beside the others (ADDONS:
header -> its entry points); EXPORTS, EXTENSION_HEADERS, EXTENSIONS and ALL_EXPORTS do not change with it.  A new
add-on is its header and its definitions; nothing is added here.

A feature added after the add-ons is a module: every .h under include/gymnast/ (MODULE_HEADERS, from the directory,
sorted, named with the directory as a C file includes them: "gymnast/newton_mpc.h", closed-loop replanning on the Newton
solver).  A module is read under the same rule (_prototypes_only) and load() binds its entry points beside the others
(MODULES: header -> its entry points); no other list changes with it, so a new module is its header and its
definitions, and nothing that pins include/'s own listing moves.

The HIP library is the only compute path of this package.  If it is missing, or no HIP
device is visible, every compute entry point raises -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import types

import torch  # noqa: F401  -- load torch's HIP runtime first so the library binds to the same one

from . import _build

# GYM_LIB_PATH selects another build of the same library (measurement / diagnostic variants)
LIB_PATH = os.environ.get("GYM_LIB_PATH") or _build.LIB_PATH

_P = C.c_void_p
# The type rule, once: a scalar goes by value; a pointer to one of the header's structs is POINTER(<that struct>);
# every other pointer, and every array declarator of a parameter (const double Q[16], gym_model out[]), is an address
# (_P).  _POINTEES are the types the header only points at.  Anything else is refused, never guessed.
_SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "int": C.c_int}
_POINTEES = ("void", "uint8_t")


def _refuse(what: str, text: str):
    raise ImportError(f"gymnast_acrobot.h: cannot bind {what}: {' '.join(text.split())!r}")


def _int(expr: str, consts: dict, what: str) -> int:
    """The value of a #define, an enumerator or an array size: digits, ( ), <<, *, +, earlier GYM_* constants and an
    LL suffix (dropped)."""
    e = re.sub(r"\bGYM_\w+", lambda m: str(consts.get(m.group(), m.group())), expr)
    e = re.sub(r"(?<=\d)LL\b", "", e)
    try:
        if not re.fullmatch(r"(?:\d+|<<|[()*+\s])+", e):
            raise SyntaxError
        return int(eval(e, {"__builtins__": {}}))
    except (SyntaxError, TypeError):         # not in the whitelist, or not an expression ("1 <<", "2 (3)")
        _refuse(what, expr)


def _decl(text: str, what: str):
    """``[const] type[*] name[size], name ...`` -> (type, is a pointer, [(name, size text or None), ...])"""
    m = re.fullmatch(r"\s*(?:const\s+)?(\w+)(\s*\*\s*|\s+)(.+?)\s*", text, flags=re.S)
    names = [re.fullmatch(r"(\w+)\s*(?:\[([^\]]*)\])?", d.strip()) for d in m.group(3).split(",")] if m else [None]
    if not all(names) or (len(names) > 1 and "*" in m.group(2)):
        _refuse(what, text)
    return m.group(1), "*" in m.group(2), [n.groups() for n in names]


def _ctype(base: str, pointer: bool, structs: dict, what: str, text: str):
    if pointer and base in structs:
        return C.POINTER(structs[base])
    if pointer and (base in _SCALARS or base in _POINTEES):
        return _P
    if not pointer and base in _SCALARS:
        return _SCALARS[base]
    _refuse(what, text)


def _parse(text: str, base=None):
    """What an ABI header's text declares: consts and status (name -> int), structs (C name -> ctypes class, fields
    in the header's order) and protos [(return type, name, [(ctypes type, parameter text), ...])] in its order.
    ``base``: the parsed header this one extends (its structs and constants are known here)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    abi = types.SimpleNamespace(consts={}, status={}, structs={}, protos=[])
    known = dict(base.structs) if base else {}
    if base:
        abi.consts.update(base.consts)
    for name, expr in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(GYM_\w+)(.*)$", text, flags=re.M):
        abi.consts[name] = _int(expr, abi.consts, f"#define {name}")
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        for item in filter(str.strip, body.split(",")):
            m = re.fullmatch(r"\s*(GYM_\w+)\s*=(.*)", item, flags=re.S)
            if not m:
                _refuse("enumerator", item)
            abi.status[m.group(1)] = _int(m.group(2), abi.consts, "enumerator")
    for body, name in re.findall(r"\btypedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
        fields = []
        for d in filter(str.strip, body.split(";")):
            what = f"field of {name}"
            base, pointer, names = _decl(d, what)
            t = _ctype(base, pointer, {**known, **abi.structs}, what, d)
            fields += [(n, t if size is None else t * _int(size, abi.consts, what)) for n, size in names]
        abi.structs[name] = type(name.title().replace("_", ""), (C.Structure,), {"_fields_": fields})
    if len(abi.structs) != len(re.findall(r"\btypedef\b", text)):
        _refuse("every typedef", "only " + " ".join(abi.structs))
    for ret, name, params in re.findall(r"^\s*(int|const\s+char\s*\*)\s+(gym_\w+)\s*\(([^()]*)\)\s*;", text,
                                        flags=re.M):
        args = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            what = f"parameter of {name}"
            base, pointer, ((_, size),) = _decl(p, what)
            t = _ctype(base, pointer or size is not None, {**known, **abi.structs}, what, p)
            args.append((t if size is None else _P, " ".join(p.split())))
        abi.protos.append(("int" if ret == "int" else "const char*", name, args))
    for name in re.findall(r"\b(gym_\w+)\s*\(", text):
        if name not in [n for _, n, _ in abi.protos]:
            _refuse("declaration of", name)
    return abi


_MAIN_HEADER = "gymnast_acrobot.h"
with open(os.path.join(_build.INCLUDE, _MAIN_HEADER)) as _f:
    _ABI = _parse(_f.read())

EXPORTS = tuple(name for _, name, _ in _ABI.protos)       # every entry point, in the header's order
_SIGS = {name: [t for t, _ in args] for _, name, args in _ABI.protos if name != "gym_build_id"}


def _prototypes_only(headers, sigs: dict) -> dict:
    """header -> its entry points for each of ``headers`` (EXTENSION_HEADERS, ADDON_HEADERS, MODULE_HEADERS), the
    signatures added to ``sigs``.  The rule for every header beside the main one, stated once: prototypes only -- no
    struct, constant or status code of its own."""
    names = {}
    for h in headers:
        with open(os.path.join(_build.INCLUDE, h)) as f:
            ext = _parse(f.read(), base=_ABI)
        if ext.structs or ext.status or ext.consts != _ABI.consts:
            _refuse("an extension header that declares more than prototypes", h)
        sigs.update({name: [t for t, _ in args] for _, name, args in ext.protos})
        names[h] = tuple(name for _, name, _ in ext.protos)
    return names


# the extensions' entry points
EXTENSION_HEADERS = tuple(sorted(f for f in os.listdir(_build.INCLUDE)
                                 if f.startswith("gymnast_acrobot_") and f.endswith(".h")))
_EXT_SIGS: dict = {}
EXTENSIONS: dict = _prototypes_only(EXTENSION_HEADERS, _EXT_SIGS)
ALL_EXPORTS = EXPORTS + tuple(_EXT_SIGS)
# the add-ons' entry points: every other header of include/ (not part of ALL_EXPORTS, whose list is ABI 18's)
ADDON_HEADERS = tuple(sorted(f for f in os.listdir(_build.INCLUDE)
                             if f.endswith(".h") and f != _MAIN_HEADER and f not in EXTENSION_HEADERS))
_ADDON_SIGS: dict = {}
ADDONS: dict = _prototypes_only(ADDON_HEADERS, _ADDON_SIGS)
# the modules' entry points: every header of include/gymnast/ (part of none of the lists above)
_MODULE_DIR = os.path.join(_build.INCLUDE, _build.MODULE_DIR)
MODULE_HEADERS = tuple(sorted(f"{_build.MODULE_DIR}/{f}" for f in (os.listdir(_MODULE_DIR) if os.path.isdir(_MODULE_DIR)
                                                                    else ()) if f.endswith(".h")))
_MODULE_SIGS: dict = {}
MODULES: dict = _prototypes_only(MODULE_HEADERS, _MODULE_SIGS)
# every GYM_<NAME> constant and status code under <NAME> (ABI_VERSION, MAX_BP, MPC_MAX_STAGES, FLAG_*, TRACK_SINGLE,
# CKPT_INTERVAL, TIMING_POOL, ...; ACTIVE ... PAD) and every struct as Gym<Name> (GymModel ... GymBatch)
globals().update({name[4:]: v for name, v in {**_ABI.consts, **_ABI.status}.items()})
globals().update({cls.__name__: cls for cls in _ABI.structs.values()})
STATUS_NAMES = {v: name[4:].lower() for name, v in _ABI.status.items()}
# the kernel kinds of gym_timing, which the header names in a comment only
KERNEL_KINDS = ("backward", "trial", "candidates", "retry", "stats", "phase_odd", "phase_even", "sigma", "run",
                "tail")
assert len(KERNEL_KINDS) == _ABI.consts["GYM_NK"]

_libs: dict = {}


def load(path: str = LIB_PATH):
    """Load (once per path) and return the ctypes library.  Raises if the HIP library is not built."""
    if path not in _libs:
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: build the HIP library first (python -m gymnast_optimalcontrol_amd._build "
                "or __graft_entry__.build()); there is no CPU fallback")
        lib = C.CDLL(path)
        lib.gym_abi_version.restype = C.c_int
        if lib.gym_abi_version() != ABI_VERSION:
            raise ImportError(f"{path} implements ABI {lib.gym_abi_version()}, this binding needs {ABI_VERSION}: "
                              "rebuild the HIP library")
        lib.gym_build_id.restype = C.c_char_p
        lib.gym_build_id.argtypes = []
        have, want = lib.gym_build_id().decode(), _build.source_hash()
        if have != want and not os.environ.get("GYM_ALLOW_FOREIGN_BUILD"):
            raise ImportError(f"{path} was built from other sources (build id {have}, tree {want}): stale binary, "
                              "rebuild it (__graft_entry__.build() or python -m gymnast_optimalcontrol_amd._build)")
        for name, args in {**_SIGS, **_EXT_SIGS, **_ADDON_SIGS, **_MODULE_SIGS}.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = C.c_int
        _libs[path] = lib
    return _libs[path]


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed with HIP error code {rc}")


def require_device(device=None, lib_path: str = LIB_PATH) -> torch.device:
    """The compute path runs on a HIP device only."""
    if not torch.cuda.is_available():
        raise RuntimeError("gymnast_optimalcontrol_amd needs a HIP (ROCm) GPU: no device is visible "
                           "and there is no CPU fallback")
    load(lib_path)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"device must be a HIP device, got {dev}")
    return dev


def ptr(t) -> int | None:
    return None if t is None else t.data_ptr()


def stream_handle(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream
