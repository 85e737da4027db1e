"""The coordinate order of the "hgx" aligner's records (hgx_align_more.order = 1, AlignIndex.align(order="coordinate"),
AlignIndex.align_resident), stated in plain Python.  It is what hgx_write_bam(sort_by_coordinate) does to the file that the
reference's pipeline stores (csrc/hgx_bam.cpp: std::stable_sort by rid, then pos0):

  - header lines ('@') stay as they are, in place;
  - body lines are stable-sorted by (index of RNAME in the header's @SQ order, POS - 1);
  - ties keep the aligner's emission order, which is read order, mate 1 before mate 2.

The host route (csrc/hgx_align_host.cpp: hgx_align_order_body) and the kernels (csrc/hgx_align.hip: k_aln_rec_keys, the radix sort,
k_aln_gather_lines) are pinned to this function byte for byte."""


def coordinate_order(sam_text):
    """`sam_text` (bytes: header lines, then one record per line, every line ending in a newline) in coordinate order (bytes)."""
    lines = sam_text.split(b"\n")
    assert lines[-1] == b"", "every line ends in a newline"
    lines.pop()
    rid = {}
    for l in lines:
        if l.startswith(b"@SQ"):
            name = [f[3:] for f in l.split(b"\t")[1:] if f.startswith(b"SN:")][0]
            rid.setdefault(name, len(rid))
    header = [l for l in lines if l.startswith(b"@")]
    body = [l for l in lines if not l.startswith(b"@")]
    assert lines == header + body, "the header stands in front of the records"

    def key(l):
        f = l.split(b"\t")
        return rid[f[2]], int(f[3]) - 1

    body.sort(key=key)                         # (list.sort is stable)
    return b"".join(l + b"\n" for l in header + body)
