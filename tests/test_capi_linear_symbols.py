"""The C-ABI of the "hgx" aligner on a linear index: declared in include/hgx.h, exported by libhgx.so, listed in capi.SYMBOLS; the
option struct's layout; the library's switch table takes the name the chunk tests lower the budgets by."""
import ctypes as C
import os
import re

from hisatgenotype_amd import align, capi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINEAR = ["hgx_align_linear_index_create", "hgx_align_linear_index_free", "hgx_align_linear_reads", "hgx_align_linear_reads_dev",
          "hgx_align_linear_last"]


def test_linear_symbols_declared_exported_and_listed():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hgx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(hgx_[a-z0-9_]+)\s*\(", src))
    lib = C.CDLL(capi.LIB_PATH)
    for n in LINEAR:
        assert n in declared and n in capi.SYMBOLS and hasattr(lib, n), n
    assert re.search(r"typedef struct hgx_align_linear_opts \{\s*int32_t bytes;[^}]*int32_t max_edits, k, fastq, route;\s*\}", src)
    assert C.sizeof(align.AlignLinearOpts) == 20 and [f for f, _ in align.AlignLinearOpts._fields_] == ["bytes", "max_edits", "k", "fastq", "route"]


def test_every_entry_cites_the_reference():
    src = open(os.path.join(ROOT, "include", "hgx.h")).read()
    block = src[src.index("the \"hgx\" aligner on a LINEAR index"):]
    for n in ("align_linear_index_create", "align_linear_reads", "align_linear_reads_dev", "align_linear_last"):
        assert re.search(re.escape(n) + r" \(typing_common\.py:610-641, 985-1056\)", block), n


def test_existing_structs_keep_their_size():
    assert C.sizeof(align.AlignOpts) == 28 and C.sizeof(align.AlignMore) == 8 and C.sizeof(align.AlignMoreOrder) == 16


def test_the_switch_table_takes_the_budget_name():
    L = capi.lib()
    L.hgx_test_switch.restype = C.c_char_p
    assert L.hgx_test_switch(b"align_linear_budget") is None
    with engine.test_switches(align_linear_budget="12,5,4"):
        assert L.hgx_test_switch(b"align_linear_budget") == b"12,5,4"
    assert L.hgx_test_switch(b"align_linear_budget") is None
