"""What the final container makes of every read (`dropest -F`): a plain restatement of FilteringBamProcessor
(Estimation/BamProcessing/FilteringBamProcessor.cpp:14-40, :61-96) and of the part of the Simple UMI merge that decides
Gene::merge_targets() when every UMI with N has one best target (MergeUMIsStrategySimple.cpp:55-102).  Written from the reference's
text; nothing here looks at the device code.  Cells are ids, genes are ids, UMIs are strings.
"""

WRITTEN, NO_GENE, CELL_NOT_KEPT, WRONG_GENE, WRONG_UMI = 0, 1, 2, 3, 4


def merge_cbs(merge_targets, filtered):
    """FilteringBamProcessor's constructor (:22-37): {cell: target} for the cells whose merge target is a filtered cell."""
    good = set(int(x) for x in filtered)
    return {b: int(t) for b, t in enumerate(merge_targets) if int(t) in good}


def decide_read(cell, gene, umi, cbs, molecules, umi_targets):
    """write_alignment (:61-96) for one read: (verdict, target cell or None, corrected UMI).
    gene: None for a read without one.  molecules: {(cell, gene): set or dict of the UMIs the gene holds in the FINAL state};
    umi_targets: {(cell, gene): {source: target}} = Gene::merge_targets()."""
    if gene is None:
        return NO_GENE, None, umi
    if cell not in cbs:
        return CELL_NOT_KEPT, None, umi
    target = cbs[cell]
    if (target, gene) not in molecules:
        return WRONG_GENE, target, umi
    sources = umi_targets.get((target, gene), {})
    if umi in sources:                        # one hop, before the molecules are asked
        return WRITTEN, target, sources[umi]
    if umi in molecules[(target, gene)]:
        return WRITTEN, target, umi
    return WRONG_UMI, target, umi


def decide_reads(cells, genes, umis, merge_targets, filtered, molecules, umi_targets):
    cbs = merge_cbs(merge_targets, filtered)
    out = [decide_read(c, g, u, cbs, molecules, umi_targets) for c, g, u in zip(cells, genes, umis)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def record_merges(log):
    """Gene::merge(source, target) with _save_merge_targets (Gene.cpp:38-58) over a log of (cell, gene, source, target) in the order
    the merges were applied: source == target is skipped (:40-41), a later assignment of a source replaces the earlier one (:56).
    Returns the rows ascending (cell, gene, source)."""
    table = {}
    for cell, gene, source, target in log:
        if source != target:
            table[(cell, gene, source)] = target
    return [(c, g, s, t) for (c, g, s), t in sorted(table.items())]


def hamming_n(a, b):
    """Tools::hamming_distance with N as a wildcard (Tools/UtilFunctions.cpp:67-82)."""
    assert len(a) == len(b)
    return sum(1 for x, y in zip(a, b) if x != y and x != "N" and y != "N")


def simple_umi_targets(group, max_ed):
    """MergeUMIsStrategySimple::find_targets (:55-102) for one (cell, gene) group {umi: reads} in which every UMI with N has exactly one
    best clean candidate: the smallest distance, then the most reads.  Returns {bad: target}; raises where the reference's answer would
    depend on its hash order or on rand() (a tie, or no candidate within max_ed)."""
    clean = [(u, r) for u, r in group.items() if "N" not in u]
    out = {}
    for bad in group:
        if "N" not in bad:
            continue
        scored = sorted((hamming_n(u, bad), -r, u) for u, r in clean)
        if not scored or scored[0][0] > max_ed:
            raise ValueError("no candidate within the distance for %s: the reference fills it at random" % bad)
        if len(scored) > 1 and scored[1][:2] == scored[0][:2]:
            raise ValueError("two best candidates for %s: the reference's pick depends on UMI index order" % bad)
        out[bad] = scored[0][2]
    return out
