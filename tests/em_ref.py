"""A plain statement of single_abundance (oracle/pyref.py:single_abundance, typing_common.py:1282-1410) with the MARGINS of
every decision it takes (TEST INFRASTRUCTURE: numpy only, no GPU, no torch).

The classes come in CSR form over any integer allele ids: `idx` (members, class after class, ascending inside a class), `off`
([C + 1] offsets) and `counts` ([C]).  Row sums are `np.add.reduceat`, column sums `np.bincount(..., weights=...)`; SQUAREM,
prob_diff, pruning from iteration index 10, the final pruning, normalisation and the optional allele lengths follow the
reference line by line.  The summation order is numpy's, not the reference's: tests/test_em_ref.py pins the result to the C
oracle within 1e-12 (same survivors, same iteration count), and on the GPU the judge is the oracle, not this file.

What this file adds to the oracle is what a test needs to know that a case is SHARP but not ambiguous:
  * margins: the smallest |p_a - max / 10| over every pruning comparison of the run and the smallest |diff - 1e-4| over every
    stopping test -- an implementation good to 1e-9 takes the same decisions when these are far above 1e-9;
  * whether `sum v^2 > 0` ever failed and whether the extrapolation was ever clamped at 0;
  * `without(...)`: the same EM with some alleles or classes taken out, to show that an element carries weight.
"""
import numpy as np

STOP = 0.0001          # common:1351
MAX_ITER = 1000
PRUNE_FROM = 10        # common:1390


class Result:
    """alleles: surviving allele ids, ascending; prob: their abundances; n_iter; first_class: lowest class index holding each
    survivor; prune_margin / stop_margin (inf when no such comparison was made); sv_failed; clamped; n_present: alleles in the
    estimate after every iteration; after_first_prune: allele ids in the estimate after iteration index 10 (None if the EM
    never got there or does not prune); first_walked: the class at which each survivor entered the LAST dict (the reference's
    result list keeps ties in that dict's order: (first_walked, key order), which is (first_class, key order) unless an earlier
    class of the allele was skipped because none of its members had a positive value)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def dense(self, n_alleles):
        """prob[n_alleles] with -1 for alleles not in the result: the form Classes.em returns"""
        out = np.full(n_alleles, -1.0)
        out[self.alleles] = self.prob
        return out


class Problem:
    def __init__(self, idx, off, counts):
        self.idx = np.ascontiguousarray(idx, np.int64)
        self.off = np.ascontiguousarray(off, np.int64)
        self.counts = np.ascontiguousarray(counts, np.int64)
        assert len(self.off) == len(self.counts) + 1 and self.off[0] == 0 and self.off[-1] == len(self.idx)
        self.size = np.diff(self.off)
        assert (self.size > 0).all(), "a class without members has no key in the reference's dict"
        self.ids, self.cidx = np.unique(self.idx, return_inverse=True)      # compact allele j is allele ids[j]
        self.n = len(self.ids)
        self.cls = np.repeat(np.arange(len(self.counts)), self.size)
        self.cnt_el = self.counts[self.cls].astype(np.float64)
        self.starts = self.off[:-1]
        self.on_step = None     # optional recorder: on_step(values [n], presence [n]) sees the INPUT of every application of the map

    # one application of the EM map (common:1311-1336) to (values, presence) over the compact alleles
    def _step(self, p, pres, ln):
        if self.on_step is not None:
            self.on_step(np.where(pres, p, 0.0), pres.copy())
        x = np.where(pres, p, 0.0)[self.cidx]
        s = np.add.reduceat(x, self.starts)
        ok = (s > 0.0)[self.cls] & pres[self.cidx]
        contrib = np.zeros(len(x))
        contrib[ok] = self.cnt_el[ok] * x[ok] / s[self.cls][ok]
        q = np.bincount(self.cidx, weights=contrib, minlength=self.n)
        qp = np.bincount(self.cidx, weights=ok, minlength=self.n) > 0
        fw = np.full(self.n, -1, np.int64)
        fw[self.cidx[ok][::-1]] = self.cls[ok][::-1]              # the class at which the allele enters the next dict
        self._first_walked = fw
        return self._norm(q, qp, ln), qp

    @staticmethod
    def _norm(q, qp, ln):
        v = np.where(qp, q if ln is None else q / ln, 0.0)
        return np.where(qp, v / v.sum(), 0.0)             # (with lengths: m / len / sum(m / len), common:1290-1297)

    def run(self, remove_low=False, lengths=None):
        """lengths: per allele ID (an array indexed by id), or None"""
        n = self.n
        ln = None if lengths is None else np.asarray(lengths)[self.ids].astype(np.float64)
        pres = np.ones(n, bool)
        p = self._norm(np.bincount(self.cidx, weights=self.cnt_el / self.size[self.cls], minlength=n), pres, ln)
        prune_margin = stop_margin = np.inf
        sv_failed = clamped = False
        n_present, after_first = [], None

        def prune(p, pres):
            nonlocal prune_margin
            if not pres.any():
                return p, pres
            thr = p[pres].max() / 10.0
            prune_margin = min(prune_margin, float(np.abs(p[pres] - thr).min()))
            keep = pres & (p >= thr)
            return np.where(keep, p, 0.0), keep

        diff, it, fw = 1.0, 0, np.full(n, -1, np.int64)
        while diff > STOP and it < MAX_ITER:
            p1, pr1 = self._step(p, pres, ln)
            fw = self._first_walked
            p2, pr2 = self._step(p1, pr1, ln)
            if (pres & ~(pr1 & pr2)).any():
                raise KeyError("reference KeyError (common:1365-1369)")
            r = np.where(pres, p1 - p, 0.0)
            v = np.where(pres, p2 - p1 - r, 0.0)
            sr, sv = float((r * r).sum()), float((v * v).sum())
            if sv > 0.0:
                g = -np.sqrt(sr / sv)
                x = p - 2 * g * r + g * g * v
                clamped |= bool((pres & (x < 0.0)).any())
                p1, pr1 = self._step(np.where(pres, np.maximum(0.0, x), 0.0), pres.copy(), ln)
                fw = self._first_walked
            else:
                sv_failed = True
            diff = float(np.where(pr1, np.abs(p - p1), p)[pres].sum())
            stop_margin = min(stop_margin, abs(diff - STOP))
            p, pres = p1, pr1
            if it >= PRUNE_FROM and remove_low:
                p, pres = prune(p, pres)
                if it == PRUNE_FROM:
                    after_first = self.ids[pres]
            n_present.append(int(pres.sum()))
            it += 1
        if remove_low:
            p, pres = prune(p, pres)
        out = self._norm(p, pres, ln)
        first = np.full(n, -1, np.int64)
        first[self.cidx[::-1]] = self.cls[::-1]                  # (the lowest class index wins the last assignment)
        return Result(alleles=self.ids[pres], prob=out[pres], n_iter=it, first_class=first[pres], prune_margin=prune_margin,
                      stop_margin=stop_margin, sv_failed=sv_failed, clamped=clamped, n_present=n_present,
                      after_first_prune=after_first, first_walked=fw[pres])

    def without(self, alleles=(), classes=()):
        """The problem with the given allele ids cleared from every class and the given classes' counts zeroed.  (A class that
        loses every member, or whose count is zero, adds nothing to any sum of the reference; it is dropped here, so class
        indices of the result are those of the smaller problem, and an allele that only such classes held leaves with them.)"""
        keep_el = ~np.isin(self.idx, np.asarray(list(alleles), np.int64))
        keep_el &= ~np.isin(self.cls, np.asarray(list(classes), np.int64))
        size = np.bincount(self.cls[keep_el], minlength=len(self.counts))
        keep_cl = size > 0
        off = np.concatenate([[0], np.cumsum(size[keep_cl])])
        return Problem(self.idx[keep_el], off, self.counts[keep_cl])


def em_ref(idx, off, counts, remove_low=False, lengths=None):
    return Problem(idx, off, counts).run(remove_low, lengths)
