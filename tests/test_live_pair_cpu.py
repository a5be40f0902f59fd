"""CPU-side checks of the pair-launch entries (dpd_gemm_f32_pair, dpd_decoder_bwd_pair_live, dpd_decoder_bwd_chain_live): the header,
lib.py and the built library agree on them, and what they refuse is refused before any device call."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dpd_gemm_f32_pair", "dpd_decoder_bwd_pair_live", "dpd_decoder_bwd_chain_live")


@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)          # hipcc cross-compiles gfx950 without a GPU
    return L.load()


def _header():
    txt = open(os.path.join(ROOT, "include", "dpdist_capi.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _prototype_args(name):
    """the argument list of `name` in the header, one C declaration per entry"""
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), flags=re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def _ctype_of(decl):
    if "*" in decl:
        for struct, cls in (("dpd_gemm_pair_part", "GemmPairPart"), ("dpd_decoder_params", "DecoderParams"), ("dpd_small_grads", "SmallGrads"),
                            ("dpd_live_rows", "LiveRows")):
            if struct in decl:
                return cls
        return "void*"
    return {"int": "int", "size_t": "size_t"}[decl.split()[0]]


def test_header_lib_py_and_library_agree_on_the_new_entries(lib):
    from dpdist_amd import lib as L
    names = {ctypes.c_int: "int", ctypes.c_size_t: "size_t", ctypes.c_void_p: "void*"}
    for n in NEW:
        assert hasattr(lib, n), "libdpdist_hip.so does not export %s" % n
        res, args = L.SIGNATURES[n]
        assert res is ctypes.c_int
        want = [_ctype_of(d) for d in _prototype_args(n)]
        got = [names[a] if a in names else a._type_.__name__ for a in args]
        assert got == want, (n, got, want)
        assert list(getattr(lib, n).argtypes) == list(args)


def test_pair_part_struct_matches_the_header():
    """field order and C types of dpd_gemm_pair_part against the ctypes mirror"""
    from dpdist_amd import lib as L
    m = re.search(r"typedef struct dpd_gemm_pair_part \{(.*?)\} dpd_gemm_pair_part;", _header(), flags=re.S)
    assert m
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ptr = "*" in decl
        for nm in decl.replace("*", " ").split(",") if not ptr else [decl.replace("*", " ")]:
            fields.append((nm.split()[-1], ctypes.c_void_p if ptr else ctypes.c_int))
    assert [(n, t) for n, t in L.GemmPairPart._fields_] == fields


def test_plan_op_of_the_pair_launch_takes_the_two_live_tiles_only(lib):
    try:
        for tile in (0, 3, 8, 30, 31, 34):
            assert lib.dpd_set_gemm_plan(12, tile, 1) == -2, tile
        assert lib.dpd_set_gemm_plan(12, 32, 1) == 0
    finally:
        assert lib.dpd_set_gemm_plan(12, 33, 1) == 0          # the plan is process-wide: back to the default
    for op in (13, 14, 15):                                    # still free
        assert lib.dpd_set_gemm_plan(op, 33, 1) < 0


def test_null_arguments_are_refused_without_a_device(lib):
    from dpdist_amd import lib as L
    part = L.GemmPairPart()
    assert lib.dpd_gemm_f32_pair(None, None, None) == -1
    assert lib.dpd_gemm_f32_pair(part, None, None) == -1
    assert lib.dpd_gemm_f32_pair(part, part, None) == -1       # NULL operands
    assert lib.dpd_decoder_bwd_pair_live(3, None, None, None, 64, 64, None, None, None) == -1
    assert lib.dpd_decoder_bwd_chain_live(*([None] * 6), 64, 96, 64, None, *([None] * 4), None, None, 0, 0, *([None] * 5), None, None) == -1
