"""The device inflate (csrc/hgx_inflate.hip) on DEFLATE streams zlib's deflate never writes: the crafted members of
tests/deflate_craft.py -- distances up to 32 768, matches at every side of the ring's constants, chains of short codes inside one
window, 15-bit codes in both alphabets, headers at the ends of their fields, every block structure -- must come out byte for byte as
the expansion of their token lists; the refused rows must be refused with the verdict the host reader's message maps to
(deflate_craft.VERDICT_OF), the members around them untouched.  Every expectation is deflate_craft.host_verdict's (zlib), which
tests/test_deflate_craft.py checks without a GPU; nothing is expected because the kernel does it.  Through hgx_bgzf_inflate_verdicts:
per-block verdicts, and 4 096 guard bytes of 0xA5 behind the payload that must come back as they were."""
import ctypes as C
import random

import numpy as np
import pytest

import deflate_craft as dc
from hisatgenotype_amd import capi

pytestmark = pytest.mark.gpu
GUARD = 4096
VALID_GROUPS = ["far_distances", "near_far_switch", "overlap", "window_chains", "code_shapes", "block_structure", "sizes", "other_encoder"]
NAMES = {v: k for k, v in vars(dc).items() if k.isupper() and isinstance(v, int) and k in
         ("OK", "BAD_BLOCK_TYPE", "BAD_STORED", "BAD_CODE", "BAD_DIST", "OVERRUN", "BAD_SIZE", "BAD_CRC", "BAD_LENGTHS", "INPUT_END")}


@pytest.fixture(autouse=True, params=[None, "inflate_small_pool", "inflate_v1"], ids=["lane_parallel", "lane_parallel_small_pool", "round4"])
def inflate_form(request):
    """Every test with the three forms of the device inflate the library holds (as tests/test_gpu_inflate.py): the default
    k_bgzf_inflate_w, the same with a second-level pool of 32 entries, and round 4's one-symbol-per-trip k_bgzf_inflate."""
    from hisatgenotype_amd import engine
    if request.param:
        engine.test_switch("front", request.param)
    yield request.param
    engine.test_switch("front", None)


def inflate_verdicts(data):
    """(output with its guard, payload bytes, [verdict per block])"""
    n_members = data.count(dc.BGZF_HEAD[:4])
    cap = 65536 * n_members + GUARD
    buf = np.zeros(cap, np.uint8)
    verdicts = np.full(n_members + 8, 0xFFFFFFFF, np.uint32)
    n_out, n_blocks = C.c_size_t(0), C.c_int64(0)
    capi.check(capi.lib().hgx_bgzf_inflate_verdicts(data, C.c_size_t(len(data)), capi.ptr(buf), C.c_size_t(cap), C.byref(n_out), capi.ptr(verdicts),
                                                    C.c_size_t(verdicts.size), C.byref(n_blocks), None))
    return buf, n_out.value, [int(v) for v in verdicts[:n_blocks.value]]


def check_file(members, form):
    """members: [(member bytes, ISIZE, expected payload or None, expected verdict, label)] -- one launch; the good members exact, the
    verdicts as expected, the guard intact."""
    buf, n_out, verdicts = inflate_verdicts(b"".join(m[0] for m in members))
    assert len(verdicts) == len(members) and n_out == sum(m[1] for m in members)
    problems, at = [], 0
    for (raw, isize, payload, want, label), got in zip(members, verdicts):
        if want == dc.ANY_BAD:
            if got == dc.OK:
                problems.append("%s: accepted" % label)
        elif got != want:
            problems.append("%s: verdict %s, expected %s" % (label, NAMES.get(got, got), NAMES[want]))
        elif payload is not None and bytes(buf[at:at + isize]) != payload:
            out = bytes(buf[at:at + isize])
            first = next(i for i in range(isize) if out[i] != payload[i])
            problems.append("%s: output differs from byte %d of %d" % (label, first, isize))
        at += isize
    assert not problems, (form, problems)
    assert (buf[n_out:n_out + GUARD] == 0xA5).all(), (form, "a write beyond the last block", int(np.flatnonzero(buf[n_out:n_out + GUARD] != 0xA5)[0]))


def as_member(c):
    return (c.member(), c.isize, c.payload, c.verdict, repr(c))


@pytest.mark.parametrize("group", VALID_GROUPS)
def test_valid_streams(group, inflate_form):
    cs = dc.cases(group, valid=True)
    assert cs
    for k in range(0, len(cs), 12):                                           # (a handful of blocks per launch)
        members = [as_member(c) for c in cs[k:k + 12]]
        check_file(members + [(dc.EOF_MEMBER, 0, b"", dc.OK, "eof")], inflate_form)
        if k == 0:
            check_file(members, inflate_form)                                 # ... and as the file's last members, nothing behind them


def test_member_at_each_offset_modulo_4(inflate_form):
    """The member's first byte at every offset modulo 4 (the readers take the stream in dwords): behind a stored member of 0 - 3
    payload bytes a member begins at 31 + k."""
    picked = [c for c in dc.case_table() if repr(c) in ("code_shapes/unary_15_bits", "far_distances/fixed", "block_structure/stored_len_%d" % (dc.T_MAX + 1),
                                                        "window_chains/independent_batch", "sizes/payload_33")]
    assert len(picked) == 5
    offsets = set()
    for c in picked:
        for k in range(4):
            lead = bytes(range(65, 65 + k))
            first = dc.good_member(lead, stored=True)
            offsets.add((len(first) + 18) % 4)
            check_file([(first, k, lead, dc.OK, "lead"), as_member(c)], inflate_form)
    assert offsets == {0, 1, 2, 3}


def _neighbours():
    rng = random.Random(77)
    a = bytes(rng.randrange(256) for _ in range(3000))
    b = bytes(rng.randrange(7) for _ in range(5000))
    return (dc.good_member(a), len(a), a, dc.OK, "good member in front"), (dc.good_member(b, stored=True), len(b), b, dc.OK, "good member behind")


REFUSED = dc.cases("refused") + dc.cases("truncated")


@pytest.mark.parametrize("case", REFUSED, ids=[c.name for c in REFUSED])
def test_refused_streams(case, inflate_form):
    """One defect per member; the member between two good ones and once more as the file's last.  The verdict is the row's -- or, where
    the row says that a form reaches another check first, that form's."""
    a, b = _neighbours()
    want = case.form_verdict.get(inflate_form, (case.verdict,))[0]
    bad = (case.member(), case.isize, None, want, repr(case))
    check_file([a, bad, b, (dc.EOF_MEMBER, 0, b"", dc.OK, "eof")], inflate_form)
    check_file([a, b, bad], inflate_form)
