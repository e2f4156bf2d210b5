"""Host logic of the continuous-batching loop (vispec_amd/model/spec_model_ours.py: specgenerate_stream) on a SIMULATED device — no GPU, no
library: the loop launches round k + 1 before it reads round k's states (one round of lookahead), so what it must get right is bookkeeping:
every request served exactly once and returned in request order with the tuple it would produce alone; a snapshot taken before a refilled
slot's new request joined is never attributed to that request; a finished request's frozen round is not counted; lookahead on and off agree.
The fake engines below execute their operations strictly in enqueue ("stream") order, like the real ones."""
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from vispec_amd.model import spec_model_ours as smo  # noqa: E402


class FakeStream:
    """The lane's stream: a FIFO of operations; `run_until(pred)` executes in order up to and including the first op satisfying pred."""

    def __init__(self, n):
        self.ops, self.n = [], n
        self.ctx = [dict(done=1, n_ctx=0, new_token=0, accept_len=0, rounds=0, tokens=[], req=None) for _ in range(n)]
        self.snap, self.ready = {}, {0: 0, 1: 0, "blocking": 0}  # ready[slot]: snapshots of that slot executed and not yet waited for
        self.rounds_executed = 0

    def _exec(self, op):
        if op[0] == "begin":
            _, t, req = op
            self.ctx[t] = dict(done=0, n_ctx=req["L"], new_token=0, accept_len=0, rounds=0, tokens=list(range(req["L"])), req=req)
        elif op[0] == "round":
            self.rounds_executed += 1
            for c in self.ctx:
                if c["done"]:
                    continue  # frozen: a finished request of a cohort (tree_kernels.h)
                r = c["req"]
                a = (r["id"] * 7 + c["rounds"] * 3) % 4  # this request's accept length in this round: a function of (request, round) only
                c["accept_len"] = a
                c["tokens"] += [1000 * r["id"] + c["new_token"] + i for i in range(a + 1)]
                c["new_token"] += a + 1
                c["n_ctx"] += a + 1
                c["rounds"] += 1
                if r["eos_round"] is not None and c["rounds"] == r["eos_round"]:
                    c["done"] |= 1
                if c["new_token"] > r["budget"]:
                    c["done"] |= 2
                if r.get("kv_full_round") is not None and c["rounds"] == r["kv_full_round"]:
                    c["done"] |= 4  # the next round would not fit a KV cache: frozen from here on, like any finished request
        elif op[0] == "snap":
            self.snap[op[1]] = [dict(n_ctx=c["n_ctx"], new_token=c["new_token"], rounds=c["rounds"], done=c["done"], accept_len=c["accept_len"],
                                     next_token=0, draft_len=0, n_leaf=0) for c in self.ctx]
            self.ready[op[1]] += 1

    def run_until(self, pred=None):
        while self.ops:
            op = self.ops.pop(0)
            self._exec(op)
            if pred is not None and pred(op):
                return
        assert pred is None, "waited for something that was never enqueued"


class FakeEngine:
    def __init__(self, stream, t, leader=None):
        self.s, self.t, self.leader, self.device = stream, t, leader, torch.device("cpu")
        self.total_token = 30

    def check_prompt_fits(self, n):
        pass

    def load_kv_rows(self, store, engines):
        pass

    def cohort_round(self, members, forced_accept=-1):
        self.s.ops.append(("round",))

    def cohort_states_enqueue(self, members, slot):
        self.s.ops.append(("snap", slot))

    def cohort_states_wait(self, members, slot):
        if not self.s.ready[slot]:  # (a blocking copy in between may already have executed it: an event that has fired)
            self.s.run_until(lambda op: op == ("snap", slot))
        assert self.s.ready[slot] == 1, "a snapshot slot was overwritten before it was read"
        self.s.ready[slot] = 0
        return self.s.snap[slot]

    def state(self):
        return self.cohort_states(())[self.t]

    def cohort_states(self, members):
        self.s.ops.append(("snap", "blocking"))  # a blocking read-back: everything enqueued before it has run
        self.s.run_until()
        return self.s.snap["blocking"]

    def tokens(self, n):
        self.s.run_until()  # a blocking copy on the stream
        return np.asarray(self.s.ctx[self.t]["tokens"][:n], np.int32)


class FakeModel:
    def __init__(self, stream, t, leader=None):
        self.engine = FakeEngine(stream, t, None if leader is None else leader.engine)
        self.spec_layer = type("S", (), dict(total_tokens=29))()
        self.current_length_data = torch.zeros(4, dtype=torch.long)
        self.base_model = SimpleNamespace(w=None, prefill=lambda x, **kw: (None, x), prefill_batch=lambda engines, xs, pos, **kw: [(None, x) for x in xs])

    def _start_request(self, ids, inputs_embeds, kw, temperature=0.0, top_k=0.0, seed=0, max_new_tokens=512, is_llama3=False):
        self.engine.s.ops.append(("begin", self.engine.t, dict(kw["req"], budget=max_new_tokens)))

    # the staged starts (batch_prefill / prefix=): the request begins in the last stage, behind the prefill stand-ins of base_model
    def _start_prepare(self, ids, inputs_embeds, kw, temperature=0.0, top_k=0.0, seed=0, max_new_tokens=512, is_llama3=False, prefix=None):
        return SimpleNamespace(req=dict(kw["req"], budget=max_new_tokens), emb=torch.zeros(ids.shape[1], 1), position_ids=None, prefix=prefix,
                               past=0 if prefix is None else prefix.rows)

    def _start_finish(self, prep, logits, hidden):
        assert hidden.shape[0] == prep.req["L"]
        self.engine.s.ops.append(("begin", self.engine.t, prep.req))

    def _visual_token_ids(self):
        return ()


def alone(req, budget, rounds_cap=10 ** 9):
    """The tuple the request produces when it runs by itself."""
    s = FakeStream(1)
    s._exec(("begin", 0, dict(req, budget=budget)))
    accs = []
    while True:
        s._exec(("round",))
        c = s.ctx[0]
        accs.append(c["accept_len"])
        if c["done"] or len(accs) >= rounds_cap:
            return c["tokens"][:c["n_ctx"]], c["new_token"], len(accs) - 1, accs


@pytest.mark.parametrize("lookahead", ["1", "0"])
@pytest.mark.parametrize("n,R", [(4, 13), (3, 7), (2, 9), (4, 5)])
def test_stream_bookkeeping_with_and_without_lookahead(monkeypatch, lookahead, n, R):
    monkeypatch.setenv("VISPEC_STREAM_LOOKAHEAD", lookahead)
    rng = np.random.default_rng(n * 100 + R)
    reqs, budgets = [], []
    for i in range(R):
        r = dict(id=i, L=int(rng.integers(5, 40)), eos_round=(int(rng.integers(1, 12)) if i % 3 == 0 else None))
        reqs.append((torch.zeros(1, r["L"], dtype=torch.long), dict(req=r)))
        budgets.append(int(rng.integers(6, 60)))
    stream = FakeStream(n)
    lead = FakeModel(stream, 0)
    models = [lead] + [FakeModel(stream, t, lead) for t in range(1, n)]
    stats = {}
    outs = smo.specgenerate_stream(models, reqs, max_new_tokens=budgets, stats=stats)
    assert len(outs) == R
    for i, (toks, new_token, idx, accs) in enumerate(outs):
        w_toks, w_new, w_idx, w_accs = alone(reqs[i][1]["req"], budgets[i])
        assert toks[0].tolist() == w_toks and (new_token, idx, accs) == (w_new, w_idx, w_accs), f"request {i}"
    assert stats["request_rounds"] == sum(len(o[3]) for o in outs)
    # lockstep rounds: the lookahead launches at most one round per refill generation more than the lockstep loop
    assert stats["rounds"] <= stream.rounds_executed <= stats["rounds"] + 1


# the sizes of the batched starts and the fan-outs of the prefix copies of the scenario below (the same with and without lookahead), recorded
# from the commit before the three start routes became one: two refills of two slots and one of a single slot, which without a prefix goes
# through _start_request and with one is a fork of its own
PREFILL_BATCHES, PREFIX_FORKS = [3, 2, 2], [3, 2, 1, 2]


@pytest.mark.parametrize("lookahead", ["1", "0"])
@pytest.mark.parametrize("prefixed", [False, True])
def test_stream_statistics_of_batched_and_prefixed_starts(monkeypatch, lookahead, prefixed):
    """3 slots, 8 requests, batch_prefill=True: budgets and EOS rounds chosen so that some refills free one slot and some free two."""
    monkeypatch.setenv("VISPEC_STREAM_LOOKAHEAD", lookahead)
    eos = [2, 2, 4, 3, 3, None, 1, None]
    budgets = [60, 50, 40, 30, 45, 9, 20, 14]
    reqs = [(torch.zeros(1, 5 + 3 * i, dtype=torch.long), dict(req=dict(id=i, L=5 + 3 * i, eos_round=eos[i]))) for i in range(8)]
    pfx = SimpleNamespace(rows=4, store=None, hidden=torch.zeros(4, 1), check_request=lambda ids, w, visual: int(ids.shape[1]))
    stream = FakeStream(3)
    lead = FakeModel(stream, 0)
    models = [lead] + [FakeModel(stream, t, lead) for t in range(1, 3)]
    stats = {}
    outs = smo.specgenerate_stream(models, reqs, max_new_tokens=budgets, stats=stats, batch_prefill=True, **({"prefix": pfx} if prefixed else {}))
    for i, (toks, new_token, idx, accs) in enumerate(outs):
        w_toks, w_new, w_idx, w_accs = alone(reqs[i][1]["req"], budgets[i])
        assert toks[0].tolist() == w_toks and (new_token, idx, accs) == (w_new, w_idx, w_accs), f"request {i}"
    assert (stats["prefill_batches"], stats.get("prefix_forks")) == (PREFILL_BATCHES, PREFIX_FORKS if prefixed else None)
    # requests <= slots: the plain cohort, one batched start
    monkeypatch.setattr(smo.torch.cuda, "current_stream", lambda *a: SimpleNamespace(synchronize=lambda: None))
    stats = {}
    smo.specgenerate_stream(models, reqs[:3], max_new_tokens=budgets[:3], stats=stats, batch_prefill=True, **({"prefix": pfx} if prefixed else {}))
    assert (stats["prefill_batches"], stats.get("prefix_forks")) == ([3], [3] if prefixed else None)


# ------------------------------------------------------------------------------------------------ specgenerate_cohort on the same fakes
def cohort_of(n):
    stream = FakeStream(n)
    lead = FakeModel(stream, 0)
    return [lead] + [FakeModel(stream, t, lead) for t in range(1, n)]


def run_cohort(monkeypatch, reqs, budgets):
    monkeypatch.setattr(smo.torch.cuda, "current_stream", lambda *a: SimpleNamespace(synchronize=lambda: None))  # `stats` brackets the loop
    stats = {}
    requests = [(torch.zeros(1, r["L"], dtype=torch.long), dict(req=r)) for r in reqs]
    return smo.specgenerate_cohort(cohort_of(len(reqs)), requests, max_new_tokens=budgets, stats=stats), stats


def same_as_alone(out, req, budget):
    toks, new_token, idx, accs = out
    w_toks, w_new, w_idx, w_accs = alone(req, budget)
    assert toks.dtype == torch.int64 and toks[0].tolist() == w_toks and (new_token, idx, accs) == (w_new, w_idx, w_accs), f"request {req['id']}"


@pytest.mark.parametrize("n", [2, 4, 8])
def test_cohort_returns_every_request_as_alone(monkeypatch, n):
    """Mixed budgets, some requests with an EOS round: every tuple is the request's own, the loop runs as long as its longest request."""
    rng = np.random.default_rng(40 + n)
    reqs = [dict(id=i, L=int(rng.integers(5, 40)), eos_round=(int(rng.integers(1, 12)) if i % 3 == 0 else None)) for i in range(n)]
    budgets = [int(rng.integers(6, 60)) for _ in range(n)]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        outs, stats = run_cohort(monkeypatch, reqs, budgets)
    for out, r, b in zip(outs, reqs, budgets):
        same_as_alone(out, r, b)
    assert len({len(o[3]) for o in outs}) > 1  # (the requests do end in different rounds)
    assert stats["rounds"] == max(len(o[3]) for o in outs)


def test_cohort_request_ended_by_a_full_kv_cache(monkeypatch):
    """A request whose state reports a full KV cache (done bit 4) without EOS or budget: one RuntimeWarning that names it, the request is
    cut there, the others complete; with EOS in the same round the request ends silently."""
    reqs = [dict(id=0, L=9, eos_round=None), dict(id=1, L=17, eos_round=None, kv_full_round=3), dict(id=2, L=30, eos_round=7)]
    budgets = [40, 50, 60]
    free = dict(reqs[1], kv_full_round=None)
    cut, whole = alone(reqs[1], budgets[1]), alone(free, budgets[1])
    assert len(cut[3]) == 3 and len(whole[3]) > 3 and cut[0] == whole[0][:len(cut[0])] and cut[1] <= budgets[1]  # alone() itself truncates there
    with pytest.warns(RuntimeWarning) as rec:
        outs, stats = run_cohort(monkeypatch, reqs, budgets)
    assert len(rec) == 1 and "cohort request 1 stopped after" in str(rec[0].message) and "KV cache" in str(rec[0].message)
    for out, r, b in zip(outs, reqs, budgets):
        same_as_alone(out, r, b)
    assert len(outs[1][3]) == 3 and stats["rounds"] == max(len(o[3]) for o in outs) > 3
    reqs[1] = dict(reqs[1], eos_round=3)  # bit 1 in the same round as bit 4
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        outs, _ = run_cohort(monkeypatch, reqs, budgets)
    assert len(outs[1][3]) == 3 and outs[1][0][0].tolist() == cut[0]


# --------------------------------------------------------------------------------------------------- the stop rule and the result builder
BUDGET = 10
# done bits: 1 = EOS, 2 = over the budget, 4 = the next round would not fit a KV cache.  The host compares new_token with its own budget (bit 2
# alone ends nothing); the warning looks at the bits (the device sets bit 2 exactly when new_token exceeds the budget it was given).
STOP_TABLE = [  # done, new_token, ended, warns
    (0, BUDGET, False, False), (0, BUDGET + 1, True, False),
    (1, BUDGET, True, False), (1, BUDGET + 1, True, False),
    (2, BUDGET, False, False), (2, BUDGET + 1, True, False),
    (4, BUDGET, True, True), (4, BUDGET + 1, True, True),
    (5, BUDGET, True, False), (5, BUDGET + 1, True, False),
    (6, BUDGET, True, False), (6, BUDGET + 1, True, False),
]


@pytest.mark.parametrize("done,new_token,ended,warns", STOP_TABLE)
def test_stop_rule(done, new_token, ended, warns):
    st = dict(done=done, new_token=new_token, n_ctx=77)
    assert smo._request_ended(st, BUDGET) is ended
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        smo._warn_kv_full(st, "request 3")
        smo._warn_kv_full(st, "specgenerate", " (context 77 of 99 rows); the returned sequence is truncated")
    assert len(rec) == (2 if warns else 0)
    if warns:
        assert all(w.category is RuntimeWarning for w in rec)
        assert str(rec[0].message) == f"request 3 stopped after {new_token} new tokens: the next round would not fit a KV cache"
        assert str(rec[1].message) == (f"specgenerate stopped after {new_token} new tokens: the next round would not fit a KV cache "
                                       "(context 77 of 99 rows); the returned sequence is truncated")


def test_result_builder():
    m = cohort_of(1)[0]
    m.engine.s._exec(("begin", 0, dict(id=5, L=6, eos_round=None, budget=20)))
    m.engine.s._exec(("round",))
    st, accs = m.engine.state(), [3, 1]
    toks, new_token, idx, got_accs = smo._request_result(m, st, 4, accs)
    assert toks.dtype == torch.int64 and tuple(toks.shape) == (1, st["n_ctx"]) and toks[0].tolist() == m.engine.s.ctx[0]["tokens"]
    assert (new_token, idx) == (st["new_token"], 4) and got_accs is accs
    assert (m.current_length_data == st["n_ctx"]).all()
