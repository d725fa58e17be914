"""The C-ABI shared library loads and exports every symbol include/rsvld_hip.h declares (no compute)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "rsvld_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rsvld_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    import ctypes
    from rsvld_amd import _lib
    names = _declared()
    assert len(names) >= 15
    assert sorted(_lib.SIGNATURES) == names, "ctypes table and header disagree"
    lib = _lib.load()
    for n in names:
        assert isinstance(getattr(lib, n), ctypes._CFuncPtr)
    assert b"gfx950" in lib.rsvld_version()


def _header_fields(name):
    """(C type, field) of ``typedef struct name { ... } name;`` in the header, in order."""
    src = open(os.path.join(ROOT, "include", "rsvld_hip.h")).read()
    start = src.index(f"typedef struct {name} {{") + len(f"typedef struct {name} {{")
    body = re.sub(r"/\*.*?\*/", "", src[start:src.index(f"}} {name};")], flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *more = decl.split(",")
        ctype = " ".join(first.split()[:-1])
        for nm in [first.split()[-1]] + more:
            fields.append((ctype, nm.strip().lstrip("*")))
    return fields


def test_conv_desc_matches_header_layout():
    """Field order / count of the ctypes struct follows the C struct declaration."""
    import ctypes
    from rsvld_amd import _lib
    assert [f for _, f in _header_fields("rsvld_conv_desc")] == [f[0] for f in _lib.ConvDesc._fields_]
    # the outputs of the host-only plan queries: field order AND integer width (Python reads them)
    widths = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    plans = (("rsvld_conv_plan", _lib.ConvPlan), ("rsvld_groupnorm_plan", _lib.GroupnormPlan),
             ("rsvld_attention_plan", _lib.AttentionPlan), ("rsvld_prefill_attention_plan", _lib.PrefillAttentionPlan),
             ("rsvld_decode_attention_mma_plan", _lib.DecodeAttentionMmaPlan), ("rsvld_gemm_w8_plan", _lib.GemmW8Plan),
             ("rsvld_gemv_mma_plan", _lib.GemvMmaPlan))
    for name, struct in plans:
        assert [(f, widths[t]) for t, f in _header_fields(name)] == list(struct._fields_), name
    # no plan struct of the header is left out of the list above
    src = open(os.path.join(ROOT, "include", "rsvld_hip.h")).read()
    assert sorted(re.findall(r"typedef struct (rsvld_\w+_plan) \{", src)) == sorted(n for n, _ in plans)


def _prototypes(src):
    """{name: (return type, [argument types])} of every function the header declares, as normalised C type strings
    (``const`` dropped, one space between words, ``*`` attached: "void*", "rsvld_conv_desc*", "int64_t")."""
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r"^\s*#[^\n]*(\\\n[^\n]*)*", "", src, flags=re.M)                    # preprocessor lines
    src = re.sub(r"typedef struct \w+ \{.*?\} \w+;", "", src, flags=re.S)
    src = src.replace('extern "C" {', "")

    def norm(t):
        words = [w for w in re.sub(r"\*", " * ", t).split() if w != "const"]
        stars = words.count("*")
        return " ".join(w for w in words if w != "*") + "*" * stars

    protos = {}
    for ret, name, args in re.findall(r"([\w\s\*]+?)\b(rsvld_\w+)\s*\(([^()]*)\)\s*;", src):
        assert name not in protos, name
        args = args.strip()
        types = []
        if args and args != "void":
            for a in args.split(","):
                m = re.fullmatch(r"\s*(.*?[\s\*])(\w+)\s*", a, flags=re.S)              # "<type> <parameter name>"
                assert m, (name, a)
                types.append(norm(m.group(1)))
        protos[name] = (norm(ret), types)
    return protos


def _ctype_of(ctype, structs):
    """The ctypes type ``_lib.SIGNATURES`` must hold for one normalised C type; ``structs``: {C struct name: ctypes.Structure}."""
    import ctypes
    scalar = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_int64, "float": ctypes.c_float}
    if ctype in scalar:
        return scalar[ctype]
    assert ctype.endswith("*") and not ctype.endswith("**"), ctype
    base = ctype[:-1]
    if base in structs:
        return ctypes.POINTER(structs[base])
    assert base in ("void", "float", "double", "char", "uint8_t", "int32_t", "int64_t", "int", "long long", "unsigned char"), ctype
    return ctypes.c_void_p


def signature_mismatches(signatures, src=None):
    """Every disagreement between a ctypes table ``{name: (restype, argtypes)}`` and the header's prototypes, as strings."""
    import ctypes
    from rsvld_amd import _lib
    if src is None:
        src = open(os.path.join(ROOT, "include", "rsvld_hip.h")).read()
    structs = {"rsvld_conv_desc": _lib.ConvDesc, "rsvld_conv_plan": _lib.ConvPlan, "rsvld_groupnorm_plan": _lib.GroupnormPlan,
               "rsvld_attention_plan": _lib.AttentionPlan, "rsvld_prefill_attention_plan": _lib.PrefillAttentionPlan,
               "rsvld_decode_attention_mma_plan": _lib.DecodeAttentionMmaPlan, "rsvld_gemm_w8_plan": _lib.GemmW8Plan,
               "rsvld_gemv_mma_plan": _lib.GemvMmaPlan}
    protos = _prototypes(src)
    bad = [f"{n}: declared on one side only" for n in sorted(set(protos) ^ set(signatures))]
    for name in sorted(set(protos) & set(signatures)):
        ret, args = protos[name]
        res, argtypes = signatures[name]
        want_res = ctypes.c_char_p if ret == "char*" else _ctype_of(ret, structs)
        if res is not want_res:
            bad.append(f"{name}: returns {ret}, the table says {res.__name__}")
        if len(args) != len(argtypes):
            bad.append(f"{name}: {len(args)} arguments in the header, {len(argtypes)} in the table")
            continue
        for i, (a, t) in enumerate(zip(args, argtypes)):
            if _ctype_of(a, structs) is not t:
                bad.append(f"{name}: argument {i} is {a}, the table says {t.__name__}")
    return bad


def test_every_prototype_matches_the_ctypes_table():
    """Return type, argument count and every argument's width of ``_lib.SIGNATURES`` follow the header: an ``int64_t`` bound as
    ``c_int`` works until a stride or an element count passes 2^31.  The check itself is shown to bite: the same table with one
    64-bit argument narrowed, one argument dropped and one return type narrowed is rejected, entry by entry."""
    import ctypes
    from rsvld_amd import _lib
    protos = _prototypes(open(os.path.join(ROOT, "include", "rsvld_hip.h")).read())
    assert len(protos) == len(_declared()) >= 90 and sorted(protos) == _declared()
    assert sum(a == "int64_t" for _, args in protos.values() for a in args) >= 60      # the parser sees the wide arguments
    assert signature_mismatches(_lib.SIGNATURES) == []
    res, args = _lib.SIGNATURES["rsvld_layernorm"]
    assert args[4] is ctypes.c_int64
    narrowed = dict(_lib.SIGNATURES, rsvld_layernorm=(res, args[:4] + [ctypes.c_int] + args[5:]),
                    rsvld_axpby=(_lib.SIGNATURES["rsvld_axpby"][0], _lib.SIGNATURES["rsvld_axpby"][1][:-1]),
                    rsvld_groupnorm_ws_bytes=(ctypes.c_int, _lib.SIGNATURES["rsvld_groupnorm_ws_bytes"][1]))
    bad = signature_mismatches(narrowed)
    assert len(bad) == 3 and "rsvld_axpby: 8 arguments in the header, 7" in bad[0] and "rsvld_groupnorm_ws_bytes: returns int64_t" in bad[1] \
        and "rsvld_layernorm: argument 4 is int64_t, the table says c_int" in bad[2], bad


def test_constants_match_header():
    """The dtype / activation / tune constants of the ctypes layer are the header's #defines (a flag added on one side only would
    silently select another kernel)."""
    from rsvld_amd import _lib
    src = open(os.path.join(ROOT, "include", "rsvld_hip.h")).read()
    defs = {}
    for name, expr in re.findall(r"^#define\s+(RSVLD_[A-Z0-9_]+)\s+(\(?-?[0-9]+(?:\s*<<\s*[0-9]+)?\)?)", src, flags=re.M):
        defs[name] = eval(expr)                      # integer literals and shifts only (the regular expression admits nothing else)
    want = {"RSVLD_F16": _lib.F16, "RSVLD_BF16": _lib.BF16, "RSVLD_F32": _lib.F32, "RSVLD_SPLIT": _lib.SPLIT,
            "RSVLD_F16W2": _lib.F16W2, "RSVLD_F16W1": _lib.F16W1, "RSVLD_F16Q8": _lib.F16Q8,
            "RSVLD_ACT_NONE": _lib.ACT_NONE, "RSVLD_ACT_SILU": _lib.ACT_SILU, "RSVLD_ACT_GEGLU": _lib.ACT_GEGLU,
            "RSVLD_TUNE_STAGES_SHIFT": _lib.TUNE_STAGES_SHIFT, "RSVLD_TUNE_NO_KSPLIT": _lib.TUNE_NO_KSPLIT,
            "RSVLD_TUNE_REG_STAGING": _lib.TUNE_REG_STAGING, "RSVLD_TUNE_HALO_NW4": _lib.TUNE_HALO_NW4,
            "RSVLD_TUNE_HALO_NW8": _lib.TUNE_HALO_NW8, "RSVLD_TUNE_NO_GEMM256": _lib.TUNE_NO_GEMM256,
            "RSVLD_TUNE_GEMM_ONE_TILE": _lib.TUNE_GEMM_ONE_TILE, "RSVLD_TUNE_F32_SPLIT": _lib.TUNE_F32_SPLIT}
    want.update({"RSVLD_ATTN_ROW_" + k.upper(): v for k, v in _lib.ATTN_ROW.items()})
    assert sum(k.startswith("RSVLD_ATTN_ROW_") for k in defs) == len(_lib.ATTN_ROW)
    for k, v in want.items():
        assert defs.get(k) == v, (k, defs.get(k), v)
    flags = [v for k, v in defs.items() if k.startswith("RSVLD_TUNE_") and k not in ("RSVLD_TUNE_TILE_MASK", "RSVLD_TUNE_STAGES_SHIFT")]
    assert len(set(flags)) == len(flags) and all(f & (f - 1) == 0 and f > 63 for f in flags), "tune flags must be distinct single bits above the tile / stage fields"
