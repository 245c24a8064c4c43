"""The ctypes signature table (``ddlw_amd/ops/abi.py``) against the
``DDLW_EXPORT`` declarations in ``ddlw_amd/ops/hip/*.hip``. Runs without a
GPU and without the built library."""
import ctypes
import re
from pathlib import Path

import pytest

from ddlw_amd.ops import abi, runtime

PKG = Path(abi.__file__).resolve().parent.parent
HIP_SOURCES = sorted((PKG / "ops" / "hip").glob("*.hip"))

C_TYPES = {
    "void*": abi.Ptr,
    "const void*": abi.Ptr,
    "int": ctypes.c_int,
    "long": ctypes.c_long,
    "float": ctypes.c_float,
    "unsigned long long": ctypes.c_ulonglong,
    "const long*": ctypes.POINTER(ctypes.c_long),
    "const int*": ctypes.POINTER(ctypes.c_int),
}
RETURN_TYPES = {"int": ctypes.c_int, "long": ctypes.c_long,
                "const char*": ctypes.c_char_p}

# exports that launch nothing and therefore take no stream
NON_LAUNCHING = {"ddlw_last_error", "ddlw_device_sync", "ddlw_bn_nparts",
                 "ddlw_depthwise_wgrad_nparts", "ddlw_conv_fwd_nparts"}

_DECL = re.compile(r"DDLW_EXPORT\s+([\w\s]+?\*?)\s*\b(ddlw_\w+)\s*\(([^)]*)\)", re.S)


def _ctype(text, table, where):
    key = re.sub(r"\s*\*", "*", " ".join(text.split()))
    assert key in table, f"{where}: unmapped C type {key!r}"
    return table[key]


def parse_exports(source: str) -> dict:
    """{name: (restype, [argtypes])} for every DDLW_EXPORT declaration."""
    out = {}
    for ret, name, params in _DECL.findall(source):
        argtypes = []
        for p in filter(None, (p.strip() for p in params.split(","))):
            ctype = re.match(r"(.*?[\s*])\w+$", p, re.S)  # drop the parameter name
            assert ctype, f"{name}: cannot parse parameter {p!r}"
            argtypes.append(_ctype(ctype.group(1), C_TYPES, name))
        assert name not in out, f"{name} declared twice"
        out[name] = (_ctype(ret, RETURN_TYPES, name), argtypes)
    return out


def mismatches(parsed: dict, table: dict) -> list:
    """Every disagreement between parsed declarations and a signature table."""
    bad = [f"{n}: exported but not in the table" for n in parsed.keys() - table.keys()]
    bad += [f"{n}: in the table but not exported" for n in table.keys() - parsed.keys()]
    for n in parsed.keys() & table.keys():
        (pret, pargs), (tret, targs) = parsed[n], table[n]
        if pret is not tret:
            bad.append(f"{n}: returns {pret.__name__}, table says {tret.__name__}")
        if len(pargs) != len(targs):
            bad.append(f"{n}: {len(pargs)} parameters, table has {len(targs)}")
            continue
        bad += [f"{n}: parameter {i} is {p.__name__}, table says {t.__name__}"
                for i, (p, t) in enumerate(zip(pargs, targs)) if p is not t]
    return sorted(bad)


@pytest.fixture(scope="module")
def parsed():
    out = {}
    for f in HIP_SOURCES:
        decls = parse_exports(f.read_text())
        # the parser must see every export: one declaration per literal marker
        assert len(decls) == f.read_text().count("DDLW_EXPORT "), f.name
        assert not out.keys() & decls.keys()
        out.update(decls)
    assert out, "no DDLW_EXPORT declarations found"
    return out


def test_table_matches_sources(parsed):
    assert mismatches(parsed, abi.SIGNATURES) == []


def test_mismatch_is_reported():
    decl = parse_exports("DDLW_EXPORT int ddlw_x(long n,\n    void* stream) {")
    assert decl == {"ddlw_x": (ctypes.c_int, [ctypes.c_long, abi.Ptr])}
    assert mismatches(decl, {"ddlw_x": (ctypes.c_int, [ctypes.c_long, abi.Ptr])}) == []
    bad = mismatches(decl, {"ddlw_x": (ctypes.c_int, [ctypes.c_int, abi.Ptr])})
    assert bad == ["ddlw_x: parameter 0 is c_long, table says c_int"]
    assert mismatches(decl, {}) and mismatches({}, {"ddlw_x": decl["ddlw_x"]})
    with pytest.raises(AssertionError, match="unmapped C type 'double'"):
        parse_exports("DDLW_EXPORT int ddlw_y(double v, void* stream)")


def test_launching_exports_end_in_stream(parsed):
    assert NON_LAUNCHING <= parsed.keys()
    for name, (_, argtypes) in parsed.items():
        if name not in NON_LAUNCHING:
            assert argtypes and argtypes[-1] is abi.Ptr, name
    for f in HIP_SOURCES:  # ... and that last pointer is named `stream`
        for _, name, params in _DECL.findall(f.read_text()):
            if name not in NON_LAUNCHING:
                assert re.search(r"void\s*\*\s*stream\s*$", params), name


def test_pw_conv_fwd_has_no_dead_parameter(parsed):
    """x, w, y, res, scale, bias, act, M, C, K, stream — no unused zero page."""
    assert len(parsed["ddlw_pw_conv_fwd"][1]) == 11
    assert len(abi.SIGNATURES["ddlw_pw_conv_fwd"][1]) == 11


def test_no_call_site_bypasses_the_table():
    own = Path(abi.__file__).resolve()
    offenders = [str(f.relative_to(PKG)) for f in sorted(PKG.rglob("*.py"))
                 if f.resolve() != own and "ctypes.c_" in f.read_text()]
    assert offenders == []


def test_symbols_resolve():
    if not runtime.has_lib():
        pytest.skip("kernel library not built")
    cdll = runtime.require_lib()
    for name, (restype, argtypes) in abi.SIGNATURES.items():
        fn = getattr(cdll, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def _column_geometry(C):
    vecC = C // 8
    VPB = min(vecC, 256)
    ROWG = 256 // VPB
    return vecC, VPB, ROWG


@pytest.mark.parametrize("C", [8, 24, 64, 2048, 2056, 4096])
@pytest.mark.parametrize("rows", [1, 9, 255, 256, 3136, 802816])
def test_partial_count_geometry_is_pinned(rows, C):
    """The partial count is part of the result (it fixes the summation
    order), so the two ``*_nparts`` queries are pinned to their formulas."""
    if not runtime.has_lib():
        pytest.skip("kernel library not built")
    vecC, VPB, ROWG = _column_geometry(C)
    need = -(-rows // ROWG)
    assert runtime.query("bn_nparts", rows, C) == min(need, 512)
    gx = -(-vecC // VPB)
    assert (runtime.query("depthwise_wgrad_nparts", rows, C)
            == max(1, min(need, max(1, 512 // gx))))


def test_depthwise_wgrad_nparts_below_one_vector():
    if not runtime.has_lib():
        pytest.skip("kernel library not built")
    for rows in (1, 256, 3136):
        assert runtime.query("depthwise_wgrad_nparts", rows, 4) == 1


def test_missing_symbol_names_it():
    class Empty:
        pass

    def missing(name):
        raise runtime.KernelLibError(f"does not export {name}")

    with pytest.raises(runtime.KernelLibError, match="ddlw_last_error"):
        abi.apply(Empty(), missing)
