"""Extractor.feed_bam on the host route (front=host, no GPU): a BAM's deflated bytes, cut anywhere, give what the lines `samtools
view` prints for its records give through the text route and the spec (tests/extract_ref.py)."""
import re

import pytest

import extract_bam_cases as X
import extract_ref


@pytest.fixture(autouse=True)
def _library():
    try:
        from hisatgenotype_amd import capi
        capi.lib()
    except (ImportError, OSError) as e:
        pytest.skip("libhgx.so does not load here: %s" % e)


def test_symbol_is_exported_and_declared():
    import os
    from hisatgenotype_amd import capi
    assert hasattr(capi.lib(), "hgx_extract_feed_bam")
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "hgx.h")).read()
    assert re.search(r"int hgx_extract_feed_bam\(hgx_extract \*h, const void \*bgzf, size_t n_bytes, int32_t last, void \*stream\);", header)


@pytest.mark.parametrize("name", X.bam_names())
def test_fixture_in_pieces(name):
    fx, regions, fams, expect = X.fixture(name)
    a = fx["args"]
    for block_size in (300, 4096):
        data = X.sam_to_bam(fx["sam"], block_size)
        for sizes in ([len(data)], [333], [1]):
            got, st, exc, _ = X.run("feed_bam", regions, fams, a, data, sizes, front="host")
            assert X.kind(exc) == fx["exception"], (block_size, sizes)
            assert {k: v.decode() for k, v in got.items()} == expect, (block_size, sizes)
            assert st["route"] == 0 and st["chunks_device"] == 0
            if exc is None:
                assert st["records"] == sum(1 for l in fx["sam"].splitlines() if l and not l.startswith("@"))
            for (f, m), text in got.items() if name != "reverse_with_n" else ():          # (its recorded files hold lower case)
                assert text.decode() == fx["files"].get(extract_ref.file_name(fx["base"], fams[f], m, a["paired"]), ""), (f, m)


def test_aux_reference_and_damage_cases():
    for case in X.CASES:
        X.check_case(case, "host", ([1 << 30], [333], [1]))


def test_file_entry_point():
    """hgx_extract_file on BAM files (Extractor.feed_file), front=host."""
    X.check_file_entry("host")
