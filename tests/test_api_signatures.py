"""CPU: the one signature table of rust_renderer_amd/api.py against the built library and include/utopian_hip.h. ctypes never compares
argtypes with a C declaration, so a row with an argument too few or too many would only show as a corrupted call; here every row is
held to the header's parameter count, to an exported symbol, and to covering every uh_* function the module names."""
import os
import re

import rust_renderer_amd as rr
from rust_renderer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "utopian_hip.h")
# parameter counts of declarations the parser below cannot read (a function-pointer parameter written in place, nested parentheses):
# none today - uh_set_restir_partition takes its callback through the typedef UhRestirExchangeFn
EXPLICIT = {}


def declared_parameter_counts():
    """{function name: number of parameters} of every uh_* declaration whose parameter list has no parentheses of its own"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    counts = {}
    for name, params in re.findall(r"\b(uh_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = params.strip()
        counts[name] = 0 if params in ("", "void") else params.count(",") + 1
    return counts


def rows():
    return {name: (row if isinstance(row, tuple) else (row, None))[0] for name, row in api._SIGNATURES.items()}


def test_the_parser_reads_the_header():
    counts = declared_parameter_counts()
    assert counts["uh_version"] == 0 and counts["uh_destroy"] == 1 and counts["uh_create"] == 4 and counts["uh_set_restir_partition"] == 5
    assert counts["uh_mgpu_create"] == 6 and counts["uh_taa_jitter"] == 2 and counts["uh_add_isosurface_mesh"] == 9
    assert len(counts) > 100


def test_no_verb_has_two_rows():
    assert not set(api._CONTEXT_VERBS) & set(api._LIBRARY_VERBS)
    assert len(api._SIGNATURES) == len(api._CONTEXT_VERBS) + len(api._LIBRARY_VERBS)


def test_every_row_names_an_exported_symbol():
    lib = rr.load_library()
    missing = [name for name in rows() if not hasattr(lib, "uh_" + name)]
    assert not missing, f"rows without a uh_ symbol in the library: {missing}"


def test_every_row_has_the_declared_number_of_arguments():
    declared = {**declared_parameter_counts(), **EXPLICIT}
    unread = [name for name in rows() if "uh_" + name not in declared]
    assert not unread, f"no declaration read from the header (add to EXPLICIT only what truly has parentheses in its parameters): {unread}"
    wrong = {name: (len(argtypes), declared["uh_" + name]) for name, argtypes in rows().items() if len(argtypes) != declared["uh_" + name]}
    assert not wrong, f"name: (argtypes, declared parameters) {wrong}"


def test_every_function_the_module_names_has_a_row():
    text = open(os.path.join(ROOT, "rust-renderer_amd", "api.py")).read()
    declared = set(declared_parameter_counts()) | set(EXPLICIT)
    named = set(re.findall(r"\buh_[a-z0-9_]+", text)) & declared
    assert len(named) > 40, "the module's text no longer names the functions it calls"
    rowless = sorted(n for n in named if n[3:] not in api._SIGNATURES)
    assert not rowless, f"named (called or documented) without a row in the signature table: {rowless}"
    # and the names it reaches through the binder are rows: _bind raises KeyError otherwise
    for name in re.findall(r"""(?:_uh|_hybrid_verb|_forward_verb)\("([a-z0-9_]+)"\)|"uh_", "([a-z0-9_]+)"\)|_hip_only\([^()]*?, "([a-z0-9_]+)"\)""", text):
        assert "".join(name) in api._SIGNATURES, name


def test_the_binder_is_the_only_place_a_signature_is_set():
    text = open(os.path.join(ROOT, "rust-renderer_amd", "api.py")).read()
    assert text.count(".argtypes") == 1 and text.count(".restype") == 1
