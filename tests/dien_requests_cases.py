"""Seeded inputs of the request-level DIEN tests (a helper, not a test): R requests with one
behaviour history each, B candidates that name their request in `request_index`.  Shared by
tests/test_gpu_dien_requests.py (the kernels) and tests/test_dien_requests_ref.py (which measures
the fp32 drift of the restatement on exactly these draws, so that the GPU tests' tolerance keeps
its meaning)."""
import functools

import torch

import dien_ref

CELLS = ("AGRU", "AUGRU")
# (R, B, T, H, nh): B = 7 and 67 leave a partly filled last wave (4 candidates per wave)
CASES = [(1, 1, 1, 16, 8), (3, 7, 3, 8, 8), (5, 67, 50, 16, 8), (2, 9, 200, 32, 16), (4, 64, 50, 16, 16)]
OP_TOL = dict(atol=1e-5, rtol=0)
VOCAB = 301
UNUSED_REQUEST = 3  # of the R = 5 case: it gets no candidate


def case_id(c):
    return "x".join(map(str, c))


@functools.lru_cache(maxsize=None)
def case(R, B, T, Hd, nh, seed=11):
    """(query [B,H], table [VOCAB,H], ids [R,T], lens [R], request_index [B], weights), CPU, never
    modified.  The first requests have the lengths 0, 1, T (1, T with two requests; T with one);
    request_index is random and unsorted, every request has a candidate wherever B allows it,
    except request UNUSED_REQUEST of the R = 5 case, which has none."""
    g = torch.Generator().manual_seed(seed + 13 * B + T + 101 * R)
    q = torch.randn(B, Hd, generator=g)
    table = torch.randn(VOCAB, Hd, generator=g)
    ids = torch.randint(0, VOCAB, (R, T), generator=g)
    lens = torch.randint(0, T + 1, (R,), generator=g)
    forced = {1: [T], 2: [1, T]}.get(R, [0, 1, T])
    lens[:len(forced)] = torch.tensor(forced)
    used = [r for r in range(R) if not (R == 5 and r == UNUSED_REQUEST)]
    req = torch.tensor(used)[torch.randint(0, len(used), (B,), generator=g)]
    if B >= len(used):  # every used request at a random place
        req[torch.randperm(B, generator=g)[:len(used)]] = torch.tensor(used)
    return q, table, ids, lens, req, tuple(dien_ref.draw_weights(Hd, nh, seed + 1))


@functools.lru_cache(maxsize=None)
def reference(R, B, T, Hd, nh, cell, dtype=torch.float64):
    """dien_ref.interest on the inputs replicated per candidate: (state [B,nh], attention [B,T]) and
    the extractor states of the R histories [R,T,nh] with rows t >= len zeroed."""
    q, table, ids, lens, req, w = case(R, B, T, Hd, nh)
    s, a, _ = dien_ref.interest(q, table[ids[req]], lens[req], w, cell, dtype)
    _, _, hs = dien_ref.interest(torch.zeros(R, Hd), table[ids], lens, w, cell, dtype)
    hs = hs * (torch.arange(T)[None, :] < lens[:, None])[:, :, None]
    return s, a, hs
