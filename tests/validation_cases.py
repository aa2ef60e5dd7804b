"""Inputs of the -S tests (test_validation_model_cpu.py, test_gpu_validation.py): small containers, how each is configured, the samples
drawn from it and the cap on draws of each.  test_validation_model_cpu.py shows on the CPU checker's container that every sample marked
`complete` finishes under the model well inside its cap, so the cap is never what makes a device comparison pass.

  planted        24 cells with barcodes of 11 and 12 bases: substitution pairs, an insertion / deletion pair across the two lengths (the last base), a
                 barcode with N beside the barcode it came from (distance 0), relatives at 2, 3 and 4 substitutions (no sample takes
                 them) and strangers, among them pairs whose banded distance is not their Levenshtein distance.  6 genes, UMIs of 4 bases.
  whitelist      poisson_cases' random_0 under a whitelist merge (-m) that folds cells; its barcodes of 10 bases come from 36 whitelist
                 entries and their neighbours.
  simple         the same stream under MERGE_SIMPLE.
  n_umis         planted's cells with N in some UMIs under the default UMI merge (random fills of N): rewritten groups.
  directional    planted's cells with UMIs one substitution apart and skewed read counts under -u: rewritten groups.
  far_apart      8 barcodes pairwise far apart: the adjacent sample finds nothing and ends at its cap.
  few_adjacent   one adjacent pair among 12 cells and a cap that ends the sample after some pairs but not all.
  one_cell, no_cell   F = 1 and F = 0.
"""
import random
from functools import lru_cache

import numpy as np

from dropest_amd import capi

import poisson_cases as pc
import validation_model as vm

ACGT = "ACGT"
DISTANT, ADJACENT = (5, 100), (1, 1)


def rnd_seq(rng, n):
    return "".join(rng.choice(ACGT) for _ in range(n))


class Case:
    """barcodes: texts (N allowed); molecules: [(cell, gene, umi text, reads)]; ctx: capi.Context keywords; parts: CONST whitelist or
    None; samples: [(min_ed, max_ed, n_pairs, max_draws, complete)]; merge: run merge_and_filter before sampling."""

    def __init__(self, name, barcodes, molecules, ctx, samples, parts=None, merge=True):
        self.name, self.barcodes, self.molecules, self.ctx, self.samples, self.parts, self.merge = name, list(barcodes), list(molecules), dict(ctx), list(samples), parts, merge
        assert len(set(self.barcodes)) == len(self.barcodes)

    def arrays(self):
        """(cb, umi, gene, aux, side strings): one gene-less read per cell first (cell id = index in barcodes), then the molecules' reads"""
        side = []

        def code(text):
            c = capi.pack_seq(text)
            if c is None:
                if text not in side:
                    side.append(text)
                c = capi.ESCAPE | side.index(text)
            return c

        cb, umi, gene = [], [], []
        umi_len = len(self.molecules[0][2]) if self.molecules else 4
        for b in self.barcodes:
            cb.append(code(b)); umi.append(code("A" * umi_len)); gene.append(capi.NO_GENE)
        for c, g, u, reads in self.molecules:
            for _ in range(reads):
                cb.append(code(self.barcodes[c])); umi.append(code(u)); gene.append(g)
        return (np.array(cb, np.uint64), np.array(umi, np.uint64), np.array(gene, np.uint32), np.full(len(cb), 2 << 16, np.uint32), side)

    def whitelist(self, directory):
        if self.parts is None:
            return None
        import whitelist_model as wm
        path = directory / (self.name + "_whitelist")
        path.write_text(wm.whitelist_text(self.parts))
        return str(path)

    def checker_kw(self, whitelist):
        """the same configuration for the CPU checker (its keyword names)"""
        k = self.ctx
        return dict(merge_kind=k.get("merge_kind", 0), barcodes_kind=k.get("barcodes_kind", 0), barcodes_file=whitelist or "",
                    min_genes_before=k.get("min_genes_before_merge", 10), min_genes_after=k.get("min_genes_after_merge", 10),
                    min_merge_fraction=k.get("min_merge_fraction", 0.2), max_cb_merge_ed=k.get("max_cb_merge_edit_distance", 2),
                    umi_merge_kind=k.get("umi_merge_kind", 0), max_umi_merge_ed=k.get("max_umi_merge_edit_distance", 1),
                    umi_mult=k.get("umi_merge_multiplier", 2.0), max_merge_prob=k.get("max_merge_prob", 1e-4),
                    max_real_merge_prob=k.get("max_real_merge_prob", 1e-7))


# ---- planted barcodes ---------------------------------------------------------------------------------------------------------------
def planted_barcodes():
    rng = random.Random(7)
    out = []
    roles = {}

    def fresh(n):
        while True:
            s = rnd_seq(rng, n)
            if all(vm.levenshtein(s, t) >= 5 for t in out):
                return s

    for k in range(3):                                       # substitution pairs, one of them between barcodes of 11 bases
        a = fresh(11 if k == 2 else 12)
        out.append(a)
        out.append(pc.sub(a, [3 + 2 * k]))
        roles["sub%d" % k] = (len(out) - 2, len(out) - 1)
    a = fresh(12)                                            # the last base missing: 12 against 11 bases.  (A base missing further in leaves the
    out += [a, a[:11]]                                       # diagonal: cell plus offset is 2 there, and a band of 1 ends the function with 2.)
    roles["indel"] = (len(out) - 2, len(out) - 1)
    a = fresh(12)                                            # N is a wildcard: distance 0
    out += [a, a[:4] + "N" + a[5:]]
    roles["n"] = (len(out) - 2, len(out) - 1)
    a = fresh(12)                                            # 2, 3 and 4 substitutions: too far for the adjacent, too near for the distant sample
    out += [a, pc.sub(a, [1, 8]), pc.sub(a, [0, 5, 10])]
    roles["near"] = (len(out) - 3, len(out) - 2, len(out) - 1)
    a = fresh(11)
    out += [a, pc.sub(a, [1, 3, 6, 9])]
    roles["near4"] = (len(out) - 2, len(out) - 1)
    a = fresh(12)                                            # a rotation: a few insertions and deletions for Levenshtein, far outside a band of 5 by row
    out += [a, a[3:] + a[:3]]
    roles["rotated"] = (len(out) - 2, len(out) - 1)
    while len(out) < 24:
        out.append(fresh(11 if len(out) % 3 == 0 else 12))
    return out, roles


def planted_molecules(seed, n_cells, umi_alphabet=ACGT):
    """6 genes, UMIs of 4 bases: most cells hold most genes, an odd cell shares half the molecules of the cell before it (non-empty
    intersections between the planted relatives), three cells hold one gene and a UMI or two (empty ones)"""
    rng = random.Random(seed)
    mol = []
    for c in range(n_cells):
        sparse = c % 8 == 7
        genes = [rng.randrange(6)] if sparse else [g for g in range(6) if rng.random() < 0.75] or [0]
        for g in genes:
            umis = set()
            while len(umis) < (rng.randint(1, 2) if sparse else rng.randint(3, 12)):
                umis.add("".join(rng.choice(umi_alphabet) for _ in range(4)))
            mol += [(c, g, u, 1) for u in sorted(umis)]
        if c % 2 == 1 and not sparse:                        # the planted relatives stand side by side: every second molecule of the cell before
            mol += [(c, g, u, 1) for k, (c0, g, u, _) in enumerate(m for m in mol if m[0] == c - 1) if k % 2 == 0 and (c, g, u, 1) not in mol]
    return mol


PLAIN = dict(merge_kind=capi.MERGE_NONE, min_genes_before_merge=1, min_genes_after_merge=1)


def planted_case():
    barcodes, roles = planted_barcodes()
    c = Case("planted", barcodes, planted_molecules(11, len(barcodes)), PLAIN,
             [DISTANT + (200, 1 << 16, True), ADJACENT + (64, 1 << 16, True)])
    c.roles = roles
    return c


def n_umis_case():
    """some UMIs carry N: the default UMI merge fills them with random bases or folds them into a neighbour -- rewritten groups"""
    barcodes, _ = planted_barcodes()
    rng = random.Random(5)
    mol = []
    for c, g, u, r in planted_molecules(12, len(barcodes)):
        if rng.random() < 0.15:
            i = rng.randrange(4)
            u = u[:i] + "N" + u[i + 1:]
        mol.append((c, g, u, r))
    mol = sorted(set(mol))
    return Case("n_umis", barcodes, mol, PLAIN, [DISTANT + (120, 1 << 16, True), ADJACENT + (32, 1 << 16, True)])


def directional_case():
    """-u: UMIs over two letters in the last two places lie one substitution apart all over; read counts of 1 to 9 let the larger absorb the smaller"""
    barcodes, _ = planted_barcodes()
    rng = random.Random(6)
    mol = []
    for c, g, u, _ in planted_molecules(13, len(barcodes)):
        u = u[:2] + "".join("AC"[ACGT.index(x) & 1] for x in u[2:])
        mol.append((c, g, u))
    mol = [(c, g, u, rng.choice((1, 1, 2, 5, 9))) for c, g, u in sorted(set(mol))]
    ctx = dict(PLAIN, umi_merge_kind=capi.UMI_MERGE_DIRECTIONAL, max_umi_merge_edit_distance=1, umi_merge_multiplier=2.0)
    return Case("directional", barcodes, mol, ctx, [DISTANT + (120, 1 << 16, True), ADJACENT + (32, 1 << 16, True)])


def _from_poisson_case(name, kind, **kw):
    c = pc.case("random_0")
    mol = [(cell, g, pc.text_of(u, c.umi_len), 1) for cell, g, u in c.molecules if g is not None]
    ctx = dict(merge_kind=kind, barcodes_kind=capi.BARCODES_CONST, min_genes_before_merge=2, min_genes_after_merge=2, **kw)
    return Case(name, c.barcodes, mol, ctx, [DISTANT + (60, 1 << 16, True), (2, 4, 24, 1 << 16, True)], parts=c.parts if kind == capi.MERGE_REAL_BARCODES else None)


def far_apart_case():
    barcodes = [ch * 12 for ch in ACGT] + ["ACACACACACAC", "GTGTGTGTGTGT", "AGAGAGAGAGAG", "CTCTCTCTCTCT"]
    return Case("far_apart", barcodes, planted_molecules(14, len(barcodes)), PLAIN, [ADJACENT + (8, 10000, False)])


def few_adjacent_case():
    """one adjacent pair (two ordered pairs of 144 candidates): 5000 draws find some tens of pairs, never 4000"""
    barcodes = planted_barcodes()[0][:2] + planted_barcodes()[0][14:24]
    return Case("few_adjacent", barcodes, planted_molecules(15, len(barcodes)), PLAIN, [ADJACENT + (4000, 5000, False)])


def small_case(name, n_cells):
    barcodes = planted_barcodes()[0][14:14 + max(n_cells, 1)]
    mol = planted_molecules(16, len(barcodes))
    ctx = dict(PLAIN) if n_cells else dict(PLAIN, min_genes_before_merge=7, min_genes_after_merge=7)   # nobody holds 7 genes: F = 0
    return Case(name, barcodes, mol, ctx, [DISTANT + (4, 1000, False), ADJACENT + (4, 1000, False)])


_CASES = {
    "planted": planted_case, "n_umis": n_umis_case, "directional": directional_case,
    "whitelist": lambda: _from_poisson_case("whitelist", capi.MERGE_REAL_BARCODES, min_merge_fraction=0.05, max_cb_merge_edit_distance=2),
    "simple": lambda: _from_poisson_case("simple", capi.MERGE_SIMPLE, min_merge_fraction=0.05, max_cb_merge_edit_distance=2),
    "far_apart": far_apart_case, "few_adjacent": few_adjacent_case,
    "one_cell": lambda: small_case("one_cell", 1), "no_cell": lambda: small_case("no_cell", 0),
}
NAMES = sorted(_CASES)
MODEL_NAMES = ["planted", "n_umis", "directional", "whitelist", "simple"]      # compared pair by pair with the model


@lru_cache(maxsize=None)
def case(name):
    c = _CASES[name]()
    assert c.name == name
    return c
