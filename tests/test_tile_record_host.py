"""CPU: what the packed tile kernel reads of a tile's plan (tile_row, tile_next, col_base, esc_ptr), restated in numpy as one row of
eight words per tile -- tests/tile_record.py -- and held to its invariants on every structure tests/test_gpu_tile_record.py
multiplies: the starts are non-decreasing, the counts even and at most 512, the owned-row ranges of successive tiles abut, zend is
not before the tile's end, packable holds exactly where packed_values.packable_tiles says so.  The structures themselves are checked
to be what their names say."""
import numpy as np
import pytest

import packed_values as pv
import tile_record as trec

TILE = pv.TILE


@pytest.mark.parametrize("kind", pv.KINDS)
@pytest.mark.parametrize("name", sorted(trec.STRUCTURES))
def test_invariants(name, kind):
    rows, cols, rp, ci = trec.STRUCTURES[name]()
    val = pv.values(kind, rp, ci)
    rec = trec.records(rp, ci, val)
    packable = trec.check_invariants(rec, rp, ci, val)
    assert packable == int(rp[-1]) // TILE - (name == "a wide tile")
    assert rec.min() >= -1 and rec.max() < 2 ** 31, "a word does not fit 32 bits"


def test_the_base_structure_has_every_kind_of_count():
    """`half` on six tiles and a tail: a wavefront without escapes beside one with 512, and odd counts that get padded."""
    rows, cols, rp, ci = pv.base()
    val = pv.values("half", rp, ci)
    rec = trec.records(rp, ci, val)
    counts = trec.counts_of(rec)
    per = pv.escapes_per_wavefront(rp, ci, val)
    assert counts[2, 0] == 0 and counts[2, 1] == 512
    assert any((p % 2 == 1).any() for p in per if p is not None)
    assert rec[6, 7] == 0 and rec[6, 1] == rows and rec[7, 4] == counts.sum()       # the partial tile; the pad holds the total
    distinct = trec.records(rp, ci, pv.values("distinct", rp, ci))
    assert np.all(trec.counts_of(distinct)[:6] == 512) and np.all(np.diff(distinct[:7, 4]) == TILE)


def test_the_record_after_a_wide_tile_does_not_depend_on_it():
    rows, cols, rp, ci = pv.base()
    val = pv.values("half", rp, ci)
    plain = trec.records(rp, ci, val)
    _, _, rp2, ci2 = pv.with_wide_tile(rows, cols, rp, ci)
    wide = trec.records(rp2, ci2, val)
    assert wide[3, 7] == 0 and wide[3, 3] == -1 and np.all(trec.counts_of(wide)[3] == 0)
    gone = int(trec.counts_of(plain)[3].sum())
    assert gone > 0
    for b in (4, 5):
        assert np.array_equal(wide[b, [0, 1, 2, 3, 5, 6, 7]], plain[b, [0, 1, 2, 3, 5, 6, 7]])
        assert wide[b, 4] == plain[b, 4] - gone                                   # only the start moves: the wide tile keeps no escapes
    assert wide[4, 4] == wide[3, 4]


def test_the_new_structures_are_what_their_names_say():
    rec = {name: trec.records(rp, ci, pv.values("half", rp, ci)) for name, (rows, cols, rp, ci) in
           ((n, f()) for n, f in trec.NEW_STRUCTURES.items())}
    assert len(rec["exactly one tile"]) == 2 and rec["exactly one tile"][0, 7] == 1
    one_more = rec["one tile and one entry"]
    assert len(one_more) == 3 and list(one_more[:2, 7]) == [1, 0]
    hole = rec["a tile in which no row starts"]
    assert hole[2, 0] == hole[2, 1] and hole[2, 7] == 1, "tile 2 owns no row and is packable all the same"
    assert hole[1, 2] - 2 * TILE == TILE + 300 and hole[1, 2] - 2 * TILE > pv.OVER   # tile 1's last row runs past tiles 2 and into 3
    short = rec["rows of one and two entries"]
    assert np.all(short[:4, 1] - short[:4, 0] > 512 + 256)
    rows, cols, rp, ci = trec.empty_rows_at_the_edges()
    edges = rec["empty rows at the tiles' edges"]
    assert len(edges) == 3 and list(edges[:2, 7]) == [1, 1]
    assert rp[edges[0, 0]] == rp[edges[0, 0] + 1] == 0                                # tile 0's first owned row is empty
    assert rp[edges[1, 0]] == rp[edges[1, 0] + 1] == TILE                             # tile 1's too
    assert edges[1, 1] == rows and rp[rows - 1] == rp[rows] == 2 * TILE               # its last owned row is empty, at offset 2048
    assert edges[1, 2] == 2 * TILE
