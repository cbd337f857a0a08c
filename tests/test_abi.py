"""CPU: the ctypes binding (reftr_amd/hip.py) against include/reftr_hip.h -- every exported symbol, every prototype's parameter
kinds, every struct field's offset and size, every constant (no compute calls) -- and the by-name descriptor builder."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "reftr_hip.h")).read(), flags=re.S)          # without comments


def declared_prototypes():
    """{function: [kind of each parameter]}; kinds: "p" pointer (any `*`, rt_stream_t, rt_comm_t), "q" 64-bit integer, "i" 32-bit
    integer, "f" float."""
    def kind(param):
        if "*" in param or "[" in param or re.search(r"\brt_(stream|comm)_t\b", param):
            return "p"
        if re.search(r"\bu?int64_t\b|\blong\b", param):
            return "q"
        return "f" if re.search(r"\bfloat\b", param) else "i" if re.search(r"\b(u?int32_t|int|unsigned)\b", param) else "?" + param
    protos = re.findall(r"\bint\s+(rt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", HEADER)
    return {name: [] if params.strip() == "void" else [kind(p) for p in params.split(",")] for name, params in protos}


def bound_kind(argtype):
    if issubclass(argtype, ctypes._Pointer) or argtype in (ctypes.c_void_p, ctypes.c_char_p):
        return "p"
    if argtype is ctypes.c_float:
        return "f"
    return {4: "i", 8: "q"}[ctypes.sizeof(argtype)]


def compile_and_run(tmp_path, body):
    """stdout lines of a C program whose main() is `body`, compiled against the header."""
    c, exe = str(tmp_path / "abi.c"), str(tmp_path / "abi")
    open(c, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "reftr_hip.h"\nint main(void){' + body + "return 0;}")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    return subprocess.check_output([exe], text=True).strip().splitlines()


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from reftr_amd import hip
    return hip


def test_every_declared_symbol_is_exported_and_bound(built):
    hip = built
    L = hip.lib()
    decl = sorted(declared_prototypes())
    assert len(decl) >= 25
    assert sorted(hip.exported_symbols()) == decl, set(hip.exported_symbols()) ^ set(decl)
    for name in decl:
        assert getattr(L, name) is not None
    assert L.rt_abi_version() == hip.ABI_VERSION


def test_prototypes_match_header(built):
    """Every prototype of the header has as many parameters as its _SIGNATURES entry, of the same kind at each position."""
    for name, kinds in declared_prototypes().items():
        restype, argtypes = built._SIGNATURES[name]
        assert restype is ctypes.c_int and [bound_kind(t) for t in argtypes] == kinds, name


def test_struct_layouts_match_header(built, tmp_path):
    """Every typedef'd struct of the header is bound, and every field of its ctypes class sits at the C compiler's offsetof with the C
    field's size (a Python field the C struct does not have fails the compile)."""
    structs = built.STRUCTS
    assert all(cls.C_NAME == name for name, cls in structs.items())
    declared = sorted(set(re.findall(r"}\s*(rt_[a-z0-9_]+)\s*;", HEADER)))
    assert len(declared) >= 36 and sorted(structs) == declared, set(structs) ^ set(declared)
    body = "".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in declared) + "".join(
        f'printf("{n}.{f} %zu %zu\\n", offsetof({n}, {f}), sizeof((({n}*)0)->{f}));' for n in declared for f, _ in structs[n]._fields_)
    facts = 0
    for line in compile_and_run(tmp_path, body):
        what, *numbers = line.split()
        name, _, field = what.partition(".")
        cls = structs[name]
        have = [ctypes.sizeof(cls)] if not field else [getattr(cls, field).offset, getattr(cls, field).size]
        assert have == [int(v) for v in numbers], (what, cls.__name__, have, numbers)
        facts += 1
    assert facts == len(declared) + sum(len(cls._fields_) for cls in structs.values())


def test_constants_match_header(built, tmp_path):
    """Every Python copy of a #define or enumerator of the header holds the header's value, under both of its names."""
    names = sorted(built.CONSTANTS)
    assert {"RT_MASK_LOSS_PARTIALS", "RT_GRAD_ACCUM_SLOTS", "RT_SQ_SLOTS", "RT_SQ_STRIDE", "RT_STATS_MAX", "RT_BATCH_STAGE_MAX_B",
            "RT_EVAL_CHUNK", "RT_DEC_MAX_LAYERS", "RT_DEC_HANDOFF_BYTES"} <= set(names)
    for prefix in ("RT_ACT_", "RT_ACCUM_", "RT_EVAL_"):          # every enumerator of the three enums
        assert {n for n in names if n.startswith(prefix)} >= set(re.findall(r"\b(%s[A-Z_]+) = " % prefix, HEADER)), prefix
    out = compile_and_run(tmp_path, "".join(f'printf("{n} %lld\\n", (long long)({n}));' for n in names))
    assert {line.split()[0]: int(line.split()[1]) for line in out} == built.CONSTANTS
    for name, value in built.CONSTANTS.items():
        assert getattr(built, name[3:]) == value, name


def test_descriptor_builder():
    """hip._set / hip._desc fill by name (no library, no GPU: a CPU tensor has an address too)."""
    from reftr_amd import hip
    x, y = torch.zeros(4), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(TypeError, match=r"LayerNormDesc \(rt_layernorm_desc\).*'colour'"):
        hip._desc(hip.LayerNormDesc, x=x, colour=1)
    d = hip._desc(hip.LayerNormDesc, x=x, gamma=None, M=3, eps=0.5)
    assert (d.x, d.gamma, d.M, d.eps) == (x.data_ptr(), None, 3, 0.5)
    assert (d.beta, d.D, d.drop_p, d.drop_seed, d.seed_dev) == (None, 0, 0.0, 0, None)          # not named: zero / NULL
    a = hip._desc(hip.AdamWDesc, p=x, range_begin=(4, 8), range_lr=[0.25], n_ranges=2)
    assert list(a.range_begin) == [4, 8, 0, 0, 0, 0, 0, 0] and list(a.range_lr) == [0.25] + [0.0] * 7 and a.n_ranges == 2
    f = hip._desc(hip.FinishDesc, src=[x, None, y], n_src=3)
    assert list(f.src)[:4] == [x.data_ptr(), None, y.data_ptr(), None]
    dec = hip.DecoderFwdDesc()
    assert hip._set(dec.layer[1], Wv=x, seed_d1=7) is not None and hip._set(dec, M=5) is dec
    raw = bytes(dec)
    at = ctypes.sizeof(hip.DecoderLayerFwd)
    assert int.from_bytes(raw[at:at + 8], "little") == x.data_ptr() and not any(raw[:at])          # layer[1].Wv set, layer[0] untouched
    assert dec.layer[1].seed_d1 == 7 and dec.layer[0].seed_d1 == 0 and dec.M == 5
    with pytest.raises(TypeError, match="rt_decoder_layer_fwd"):
        hip._set(dec.layer[0], t32=x)          # a field of the parent, not of the layer


def test_library_missing_fails_loudly(monkeypatch):
    from reftr_amd import hip
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setattr(hip, "LIB_PATH", "/nonexistent/libreftr_hip.so")
    with pytest.raises(RuntimeError, match="not built"):
        hip.lib()
