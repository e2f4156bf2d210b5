"""Host-side planning of a chunked prompt prefill (TargetLM.prefill / prefill_batch with chunk_rows).  Pure Python: no torch, no GPU."""
from __future__ import annotations


def plan_prefill_pieces(lens, chunk_rows, max_segments=8, past_lens=None):
    """Cut the concatenated row stream of prompts of `lens` rows into consecutive pieces of at most `chunk_rows` rows and `max_segments`
    segments each.  -> [[(request, row0_in_piece, pos0, len), ...], ...]: rows [row0_in_piece, row0_in_piece + len) of the piece are rows
    [pos0, pos0 + len) of prompt `request` — pos0 = the rows of that prompt already placed in earlier pieces.  A piece may hold the tail of
    one prompt, whole prompts and the head of the next; a prompt's rows are consecutive in the stream, so it has at most one segment per
    piece.  Within a piece the segments are ascending and packed (row0 of a segment = the end of the one before it).
    past_lens = [P_r, ...] (one per prompt, optional): `lens` then counts the NEW rows of prompt r only — the rows behind P_r cache rows that
    are already live (a shared prompt prefix) — and pos0 = P_r + the new rows already placed.  None is all zeros: the output is unchanged."""
    lens = [int(ln) for ln in lens]
    past = [0] * len(lens) if past_lens is None else [int(p) for p in past_lens]
    if len(past) != len(lens) or any(p < 0 for p in past):
        raise ValueError("plan_prefill_pieces: one non-negative past length per prompt")
    chunk_rows, max_segments = int(chunk_rows), int(max_segments)
    if chunk_rows < 1 or max_segments < 1:
        raise ValueError("plan_prefill_pieces: chunk_rows and max_segments must be positive")
    if any(ln < 1 for ln in lens):
        raise ValueError("plan_prefill_pieces: every prompt has at least one row")
    pieces, cur, rows = [], [], 0
    for r, ln in enumerate(lens):
        done = 0
        while done < ln:
            if rows == chunk_rows or len(cur) == max_segments:
                pieces.append(cur)
                cur, rows = [], 0
            take = min(ln - done, chunk_rows - rows)
            cur.append((r, rows, past[r] + done, take))
            rows += take
            done += take
    if cur:
        pieces.append(cur)
    return pieces
