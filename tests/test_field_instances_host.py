"""The parameter lists of tests/test_gpu_field_instances.py, host side (no GPU): from the two rules restated there
(``nf -> MAXT``, ``nf -> NFT``) the derived ``(k, ncomp)`` list reaches every compiled instance of ``k_mode_project`` and of
``k_mode_project_sampled`` at its smallest and at its largest reachable field count; the restated rules, value lists and
constants are the ones of ``csrc/kernels_fields.hip`` (read as text); and the shapes of the group, regime and small-mesh
tests are in the regime their names say."""
import os
import re

import test_gpu_field_instances as fi
from pl_fem_vectoriel_amd.fields import PROJECT_SAMPLED_MAX_FRAMES, PROJECT_SAMPLED_TILE, PROJECT_TILE

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pl_fem_vectoriel_amd", "csrc", "kernels_fields.hip")
# written down by hand from the two rules, as a check of the derivation: pairs the derived list must contain, besides the
# six pairs of the two projection test files
EXPECTED = ((8, 1), (9, 1), (8, 2), (16, 1), (17, 1), (12, 2), (25, 1), (32, 1), (20, 2), (41, 1), (48, 1), (24, 2), (49, 1), (28, 2),
            (57, 1), (40, 2), (41, 2), (48, 2), (49, 2), (56, 2), (57, 2))


def _source():
    with open(SOURCE) as f:
        return f.read()


def _constant(text, name):
    m = re.search(rf"constexpr int {name} = (\d+);", text)
    assert m, name
    return int(m.group(1))


def _instances(text, plan_field):
    """The value list of the with_constant<...>(plan.<field>, ...) dispatch."""
    m = re.search(rf"with_constant<([0-9, ]+)>\(plan\.{plan_field},", text)
    assert m, plan_field
    return tuple(int(v) for v in m.group(1).split(","))


def test_the_restated_lists_and_constants_are_the_sources():
    text = _source()
    assert _instances(text, "maxt") == fi.MAXT_COMPILED and _instances(text, "nft") == fi.NFT_COMPILED
    assert "template <int MAXT>              // most fields per wave: ncomp k <= 4 MAXT" in text
    assert "template <int NFT>                   // field tiles: ncomp k <= 16 NFT" in text
    for name, value in (("PJ_SLICES", fi.PJ_SLICES), ("PJ_WG", fi.PJ_WG), ("PJ_KMAX", fi.KMAX), ("QKMAX", fi.KMAX),
                        ("PS_SLICES", fi.PS_SLICES), ("PS_GROUP", fi.PS_GROUP), ("QP", fi.QP), ("QB_MAX", fi.QB_MAX),
                        ("QWG", fi.QWG), ("PJ_X", PROJECT_TILE[0]), ("PJ_Y", PROJECT_TILE[1]), ("PS_F", PROJECT_SAMPLED_TILE),
                        ("PS_FRAMES", PROJECT_SAMPLED_MAX_FRAMES)):
        assert _constant(text, name) == value, name
    # the rules as the host code writes them
    assert "p.maxt = (p.nf + 3) / 4;" in text and "p.maxt += p.maxt <= 16 ? p.maxt % 2 : (4 - p.maxt % 4) % 4;" in text
    assert "p.nft = (p.nf + 15) / 16;" in text and "if (p.nft == 5) p.nft = 6;" in text and "if (p.nft == 7) p.nft = 8;" in text
    assert "p.slices = (int)std::max<int64_t>(1, std::min<int64_t>(PJ_SLICES, PJ_WG / p.tiles));" in text
    assert "std::max(1, std::min(QB_MAX, QWG / quartic_tile_pairs(k)))" in text


def test_the_rules_pick_the_smallest_instance_that_holds_the_fields():
    """``ncomp k <= 4 MAXT`` and ``ncomp k <= 16 NFT``, with the smallest compiled value for which that holds: never a value
    outside the list, for which the dispatch would fall through to its last instance."""
    assert fi.REACHABLE[0] == 1 and fi.REACHABLE[-1] == 2 * fi.KMAX
    for nf in range(1, 2 * fi.KMAX + 1):
        assert fi.maxt_of(nf) == min(v for v in fi.MAXT_COMPILED if nf <= 4 * v), nf
        assert fi.nft_of(nf) == min(v for v in fi.NFT_COMPILED if nf <= 16 * v), nf


def test_the_pairs_reach_every_instance_at_both_ends():
    pairs = fi.INSTANCE_PAIRS
    assert len(set(pairs)) == len(pairs)
    assert all(1 <= k <= fi.KMAX and ncomp in (1, 2) for k, ncomp in pairs)
    have = {k * ncomp for k, ncomp in pairs}
    for rule, values in ((fi.maxt_of, fi.MAXT_COMPILED), (fi.nft_of, fi.NFT_COMPILED)):
        for v in values:
            nfs = [nf for nf in fi.REACHABLE if rule(nf) == v]
            assert nfs, v                                          # every compiled value can be reached
            assert min(nfs) in have and max(nfs) in have, (rule.__name__, v, min(nfs), max(nfs))
        assert {rule(k * ncomp) for k, ncomp in pairs} == set(values)
    # the upper end is the instance's own edge wherever a call can have that count
    for v in fi.MAXT_COMPILED:
        assert 4 * v in have or 4 * v not in fi.REACHABLE, v
    for v in fi.NFT_COMPILED:
        assert 16 * v in have, v
    assert set(EXPECTED) <= set(pairs) and set(fi.ALREADY) <= set(pairs)
    # both record kinds at every count that both can have
    assert all((nf, 1) in pairs and (nf // 2, 2) in pairs for nf in have if nf % 2 == 0 and nf <= fi.KMAX and nf in fi.EDGES)
    print(len(pairs), "pairs:", pairs)


def test_the_bit_comparisons_cross_instances():
    for ncomp, ks in fi.BITS_K.items():
        assert ks[-1] == fi.KMAX and list(ks) == sorted(set(ks))
        inst = [(fi.maxt_of(ncomp * k), fi.nft_of(ncomp * k)) for k in ks]
        assert len({m for m, _ in inst}) >= 8 and len({n for _, n in inst}) >= 4, (ncomp, inst)
    assert {fi.nft_of(ncomp * k) for ncomp, ks in fi.BITS_K.items() for k in ks} == set(fi.NFT_COMPILED)
    assert len({fi.maxt_of(ncomp * k) for ncomp, ks in fi.BITS_K.items() for k in ks}) == len(fi.MAXT_COMPILED)


def test_the_shapes_are_in_their_regimes():
    T, G = PROJECT_SAMPLED_TILE, fi.PS_GROUP
    tiles = [-(-nf // T) for nf in fi.GROUP_COUNTS]
    assert fi.GROUP_COUNTS == (512, 513, 544, 547) and tiles == [G, G + 1, G + 1, G + 2]
    assert fi.GROUP_COUNTS[3] % T != 0 and PROJECT_SAMPLED_MAX_FRAMES == 8 * G * T
    TX, TY = PROJECT_TILE
    grids = {(la, lb): (-(-la // TX), -(-lb // TY)) for la, lb in fi.REGIMES}
    assert grids == {(184, 184): (23, 23), (264, 250): (33, 32), (3, 320): (1, 40), (320, 3): (40, 1)}
    assert fi.project_slices(184, 184) == 1 and 23 * 23 > fi.PJ_WG // 2
    assert fi.project_slices(264, 250) == 1 and fi.PJ_WG // (33 * 32) == 0
    assert fi.project_slices(21, 19) == 113                        # the largest table of test_gpu_projection.py
    # fewer elements than slices
    for n in fi.SMALL_N:
        assert all(2 * n * n < fi.project_slices(la, lb) for la, lb in fi.SMALL_COUNTS) and 2 * n * n < fi.PS_SLICES
    assert [fi.quartic_slices(k) for k in (1, 12, 64)] == [128, 128, 3]
    assert set(fi.QUARTIC_CASES) == {(1, 1), (1, 12), (1, 64), (2, 1), (2, 12), (5, 1), (5, 12)}
