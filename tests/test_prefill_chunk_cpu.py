"""CPU (no GPU, no torch): plan_prefill_pieces, the cutting of a batch's concatenated row stream into the pieces of a chunked prefill."""
import pytest

import helpers  # noqa: F401  (puts the repository root on sys.path)

LENS = [(300,), (129, 128, 127), (2704, 1584, 911, 640, 257, 129, 64, 1), (4,) * 9]


def chunk_sizes(lens):
    return [1, 37, 128, 129, 1000, sum(lens), sum(lens) + 5]


@pytest.mark.parametrize("lens", LENS)
def test_pieces_cover_every_row_once_in_order(lens):
    from vispec_amd.prefill_plan import plan_prefill_pieces
    for C in chunk_sizes(lens):
        pieces = plan_prefill_pieces(lens, C)
        placed = [0] * len(lens)
        stream = []  # (request, prompt row) in the order the pieces hold them
        for piece in pieces:
            assert 1 <= len(piece) <= 8, (lens, C)
            end = 0
            for r, row0, pos0, ln in piece:
                assert ln >= 1 and row0 >= end, "row0 ascending and disjoint"
                assert row0 == end, "segments are packed"
                assert pos0 == placed[r], "pos0 = the rows of that request already placed"
                end = row0 + ln
                placed[r] += ln
                stream += [(r, pos0 + k) for k in range(ln)]
            assert end <= C, "piece rows <= chunk_rows"
            assert len({r for r, *_ in piece}) == len(piece), "one segment per request and piece"
        assert placed == list(lens)
        assert stream == [(r, k) for r, ln in enumerate(lens) for k in range(ln)], "every row exactly once, in order"
        if len(lens) <= 8:  # nothing forces an early cut: every piece but the last is full
            assert all(sum(s[3] for s in piece) == C for piece in pieces[:-1])
            assert len(pieces) == -(-sum(lens) // C)


def test_more_than_eight_prompts_cut_at_eight_segments():
    from vispec_amd.prefill_plan import plan_prefill_pieces
    pieces = plan_prefill_pieces((4,) * 9, 1000)
    assert [len(p) for p in pieces] == [8, 1] and pieces[1] == [(8, 0, 0, 4)]
    assert [len(p) for p in plan_prefill_pieces((4,) * 9, 1000, max_segments=2)] == [2, 2, 2, 2, 1]


def test_a_piece_holds_tail_whole_prompts_and_head():
    from vispec_amd.prefill_plan import plan_prefill_pieces
    assert plan_prefill_pieces((5, 2, 6), 4) == [[(0, 0, 0, 4)], [(0, 0, 4, 1), (1, 1, 0, 2), (2, 3, 0, 1)], [(2, 0, 1, 4)], [(2, 0, 5, 1)]]


def test_bad_arguments_are_refused():
    from vispec_amd.prefill_plan import plan_prefill_pieces
    for lens, C in (((3,), 0), ((3,), -1), ((3, 0), 2)):
        with pytest.raises(ValueError):
            plan_prefill_pieces(lens, C)
    assert plan_prefill_pieces((), 5) == []


def test_the_planner_does_not_import_torch():
    import os
    import re
    src = open(os.path.join(helpers.ROOT, "vispec_amd", "prefill_plan.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(torch|numpy|\.)", src, flags=re.M)
