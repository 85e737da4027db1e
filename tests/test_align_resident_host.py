"""Coordinate order on the host route of the "hgx" aligner (csrc/hgx_align_host.cpp: hgx_align_order_body, hgx_align_more.order
through hgx_align_reads_x, route forced with front=host): align(order="coordinate") is the statement (tests/align_resident_ref.py)
applied to align(), byte for byte, in every form of the call; the counters do not move; the field's versions (bytes = 8 / 12 / 16)
and the refused value; inputs where only stability decides or nothing aligns; the BAM of the ordered text against the file route's;
the stand-alone host program under the sanitizers.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

import align_cases
import align_rescue_cases as rc
from align_resident_ref import coordinate_order
from hisatgenotype_amd import align, bamio, capi, engine, simulate
from test_align_rescue_host import _write_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = rc.INPUT_IDS + align_cases.INPUT_IDS
FORMS = {"default": {}, "states_all": dict(search="states_all"), "pair_aware": dict(pair="aware"), "clip": dict(clip=32),
         "gap": dict(gap=16), "rescue": dict(rescue=(16, 32))}
MAIN_ARGS = {"default": [], "states_all": ["search=2"], "pair_aware": ["pair=1"], "clip": ["clip=32"], "gap": ["gap=16"],
             "rescue": ["rescue=16,32"]}


def _host(ix, texts, me, **kw):
    with engine.test_switches(front="host"):
        out = ix.align(texts, max_edits=me, **kw)
    last = align.align_last()
    assert last["route"] == 0 and last["decline"] == align.DECLINE_SWITCH
    return out, last


_PLAIN = {}


def plain_text(form, key):
    """align() of input `key` in form `form` on the host route (bytes) and its counters, computed once per process."""
    if (form, key) not in _PLAIN:
        d, texts, me, _, _ = rc._input(key)
        ix = align.AlignIndex(*d)
        try:
            _PLAIN[(form, key)] = _host(ix, texts, me, **FORMS[form])
        finally:
            ix.close()
    return _PLAIN[(form, key)]


@pytest.mark.parametrize("form", list(FORMS))
def test_coordinate_order_is_the_statement_applied_to_read_order(form):
    moved = 0
    for key in KEYS:
        d, texts, me, _, _ = rc._input(key)
        plain, last0 = plain_text(form, key)
        ix = align.AlignIndex(*d)
        try:
            got, last1 = _host(ix, texts, me, order="coordinate", **FORMS[form])
        finally:
            ix.close()
        want = coordinate_order(plain)
        assert got == want, key
        assert last1 == last0, key                           # every counter of align_last(): the order moves none
        moved += want != plain
    assert moved > 10                                        # (the inputs do have records out of coordinate order)


class More8(C.Structure):
    _fields_ = [("bytes", C.c_int32), ("gap", C.c_int32)]


class More16(C.Structure):
    _fields_ = [("bytes", C.c_int32), ("gap", C.c_int32), ("rescue_clip", C.c_int32), ("order", C.c_int32)]


def _raw(ix, text, more):
    o = align.AlignOpts(2, 1000, -1, 1, 0, 0, 0)
    out_p, n = C.c_void_p(), C.c_size_t(0)
    bufs = (C.c_char_p * 1)(text)
    sizes = (C.c_size_t * 1)(len(text))
    rc_ = capi.lib().hgx_align_reads_x(ix.h, C.c_int32(1), None, bufs, sizes, C.byref(o), C.byref(more), C.byref(out_p), C.byref(n))
    if rc_:
        return rc_, capi.lib().hgx_last_error().decode()
    try:
        return 0, C.string_at(out_p.value, n.value)
    finally:
        capi.lib().hgx_free_text(out_p)


def test_the_versions_of_the_field():
    """`order` is read only from bytes = 16 on: the 16-byte struct under bytes = 8 or 12 gives read order whatever the word holds;
    bytes = 16 reads it; 2 and -1 are refused with the field's name."""
    d, texts, me = align_cases.inputs()["single-fastq"]
    ix = align.AlignIndex(*d)
    try:
        plain = ix.align(texts, max_edits=me, route="host")
        want = coordinate_order(plain)
        assert want != plain
        assert _raw(ix, texts[0], More8(8, 0)) == (0, plain)
        for word in (0, 1, 2, -7):
            assert _raw(ix, texts[0], More16(8, 0, 0, word)) == (0, plain)
            assert _raw(ix, texts[0], More16(12, 0, 0, word)) == (0, plain)
        assert _raw(ix, texts[0], More16(16, 0, 0, 0)) == (0, plain)
        assert _raw(ix, texts[0], More16(16, 0, 0, 1)) == (0, want)
        for bad in (2, -1):
            code, msg = _raw(ix, texts[0], More16(16, 0, 0, bad))
            assert code == -1 and "(order)" in msg
        assert ix.align(texts, max_edits=me, route="host", order=1) == want
        with pytest.raises(capi.HgxError, match="order"):
            ix.align(texts, max_edits=me, route="host", order=2)
        with pytest.raises(KeyError):
            ix.align(texts, max_edits=me, route="host", order="name")
    finally:
        ix.close()


def test_only_stability_decides():
    """The same read name twice and a third read, all placed at one position, then a read left of them: the three keep the order
    they were given in, the fourth goes in front."""
    loc = align_cases.length_locus()
    d = align_cases.dicts_of([loc])
    reads = [("twin", loc.bb[500:600]), ("twin", loc.bb[500:620]), ("other", loc.bb[500:560]), ("left", loc.bb[100:180])]
    for perm in ([0, 1, 2, 3], [1, 0, 2, 3], [2, 1, 0, 3], [3, 2, 0, 1]):
        text = align_cases.fasta([reads[k] for k in perm])
        ix = align.AlignIndex(*d)
        try:
            plain, _ = _host(ix, [text], 2)
            got, _ = _host(ix, [text], 2, order="coordinate")
        finally:
            ix.close()
        lines = plain.split(b"\n")[1:-1]
        assert [l.split(b"\t")[3] for l in lines] == [b"101" if k == 3 else b"501" for k in perm]
        assert got == coordinate_order(plain)
        body = got.split(b"\n")[1:-1]
        assert body[0] == lines[perm.index(3)] and body[1:] == [l for k, l in zip(perm, lines) if k != 3]
        assert [len(l.split(b"\t")[9]) for l in body[1:]] == [{0: 100, 1: 120, 2: 60}[k] for k in perm if k != 3]


def test_no_aligned_read_gives_the_header_alone():
    loc = align_cases.length_locus()
    ix = align.AlignIndex(*align_cases.dicts_of([loc]))
    try:
        junk = align_cases.fasta([("j%d" % k, align_cases.rand_seq(__import__("random").Random(k), 80)) for k in range(5)])
        for text in (junk, b""):
            got, last = _host(ix, [text], 2, order="coordinate")
            assert got == b"@SQ\tSN:%s\tLN:%d\n" % (loc.name.encode(), len(loc.bb)) and last["aligned"] == 0
    finally:
        ix.close()


def _refs(text):
    return [(f[1][3:].decode(), int(f[2][3:])) for f in (l.split(b"\t") for l in text.split(b"\n") if l.startswith(b"@SQ"))]


@pytest.mark.parametrize("key", ["pairs_two_genes-2", "single-fastq", "mixed-err1"])
def test_the_bam_of_the_ordered_text_is_the_file_routes(key, tmp_path):
    """hgx_write_bam WITHOUT its sort over coordinate_order(text) holds the records, in the order, of the file that the file route
    stores (simulate._store_as_the_reference_does: hgx_write_bam with its sort over the text in read order)."""
    plain, _ = plain_text("default", key)
    ordered = coordinate_order(plain)
    body = b"".join(l + b"\n" for l in ordered.split(b"\n") if l and not l.startswith(b"@"))
    bamio.write_bam_native(str(tmp_path / "ordered.bam"), body.decode(), _refs(plain), sort_by_coordinate=False)
    simulate._store_as_the_reference_does(str(tmp_path / "file_route.bam"), plain.decode())
    got = bamio.read_bam(str(tmp_path / "ordered.bam"))
    assert got == bamio.read_bam(str(tmp_path / "file_route.bam")) and len(got) == body.count(b"\n") > 10


def test_the_stand_alone_host_program_under_asan_and_ubsan(tmp_path):
    """tools/align_host_main.cpp with order=coordinate, built with -fsanitize=address,undefined (a program with its own main; nothing
    of the GPU library, nothing loaded into Python): the statement applied to the library's read-order text, and no sanitizer
    report, on every input in the default form and on the rescue inputs in every other form they take."""
    exe = str(tmp_path / "align_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DHGX_ALIGN_STANDALONE", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "hisat-genotype_amd", "csrc"),
                           os.path.join(ROOT, "hisat-genotype_amd", "csrc", "hgx_align_host.cpp"), os.path.join(ROOT, "tools", "align_host_main.cpp"),
                           "-lz", "-o", exe])
    done = 0
    for form in FORMS:
        for key in (KEYS if form == "default" else rc.INPUT_IDS):
            d, texts, me, _, _ = rc._input(key)
            ix = str(tmp_path / (key + ".ix"))
            _write_index(ix, d)
            paths = []
            for m, t in enumerate(texts):
                paths.append(str(tmp_path / ("%s_%d.in" % (key, m))))
                with open(paths[-1], "wb") as f:
                    f.write(t)
            r = subprocess.run([exe, ix, str(me)] + paths + MAIN_ARGS[form] + ["order=coordinate"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert r.returncode == 0 and r.stderr == b"", (form, key, r.stderr[-2000:])
            assert r.stdout == coordinate_order(plain_text(form, key)[0]), (form, key)
            done += 1
    assert done == len(KEYS) + 5 * len(rc.INPUT_IDS)
