"""Restatement of DIEN's eval forward ("DIEN"; reference algorithm/DIEN/dien.py:198-254,
custom_grucell.py:19-167, rnn.py:201-219) in plain torch ops, one Python loop step per time step.
A helper, not a test: float64 on the CPU is the oracle of tests/test_dien_host.py and
tests/test_gpu_dien.py; with dtype=float32 on a GPU the same loop is the eager baseline
tools/dien_time.py times.  torch.nn.GRU is deliberately not used: TF's GRUCell multiplies the
state by the reset gate before the candidate matmul, torch's after it.
"""
from __future__ import annotations

import torch

WEIGHT_NAMES = ("Wg", "bg", "Wc", "bc", "A", "Vg", "vg", "Vc", "vc")
PAD = float(-2 ** 32 + 1)
SEQ_KEY = "his_read_comment_7d_seq"
CATEGORY = ("userid", "device", "authorid", "bgm_song_id", "bgm_singer_id", "manual_tag_list")


def _gates(x, state, Wg, bg, Wc, bc):
    """TF GRUCell's gates: returns (u, c)."""
    nh = state.shape[1]
    ru = torch.sigmoid(torch.cat([x, state], 1) @ Wg.T + bg)
    r, u = ru[:, :nh], ru[:, nh:]
    c = torch.tanh(torch.cat([x, r * state], 1) @ Wc.T + bc)
    return u, c


def interest(query, keys, lengths, weights, cell_type="AGRU", dtype=torch.float64):
    """query [B,H], keys [B,T,H], lengths [B], weights = (Wg, bg, Wc, bc, A, Vg, vg, Vc, vc)
    -> (final_state [B,nh], attention [B,T], hidden states [B,T,nh])."""
    if cell_type not in ("AGRU", "AUGRU"):
        raise ValueError(cell_type)
    Wg, bg, Wc, bc, A, Vg, vg, Vc, vc = [w.to(dtype) for w in weights]
    query, keys = query.to(dtype), keys.to(dtype)
    B, T, _ = keys.shape
    nh = A.shape[0]
    # interest extractor: GRUCell over all T steps (the reference passes no sequence_length)
    h = torch.zeros(B, nh, dtype=dtype, device=keys.device)
    hs = []
    for t in range(T):
        u, c = _gates(keys[:, t], h, Wg, bg, Wc, bc)
        h = u * h + (1 - u) * c
        hs.append(h)
    hs = torch.stack(hs, 1)
    # attention: s_t = h_t . (A e_target), padded positions at -2^32+1, softmax over all T
    mask = torch.arange(T, device=keys.device)[None, :] < lengths.to(keys.device)[:, None]
    score = torch.einsum("btn,bn->bt", hs, query @ A.T)
    att = torch.softmax(torch.where(mask, score, torch.full_like(score, PAD)), 1)
    # interest evolution: t < len only, the state is copied through past len
    s = torch.zeros(B, nh, dtype=dtype, device=keys.device)
    for t in range(T):
        u, c = _gates(hs[:, t], s, Vg, vg, Vc, vc)
        a = att[:, t:t + 1]
        if cell_type == "AGRU":
            new = (1 - a) * s + a * c
        else:
            u = (1 - a) * u
            new = u * s + (1 - u) * c
        s = torch.where(mask[:, t:t + 1], new, s)
    return s, att, hs


def model_weights(p):
    """The nine interest weights out of a rankops.DIEN state_dict."""
    return (p["gru.gates.weight"], p["gru.gates.bias"], p["gru.candidate.weight"], p["gru.candidate.bias"],
            p["attention_project_matrix"], p["evolution.gates.weight"], p["evolution.gates.bias"],
            p["evolution.candidate.weight"], p["evolution.candidate.bias"])


def _bn_eval(x, p, prefix, affine, eps=1e-5):
    y = (x - p[prefix + "running_mean"]) / torch.sqrt(p[prefix + "running_var"] + eps)
    return y * p[prefix + "weight"] + p[prefix + "bias"] if affine else y


def forward(p, dense, category, sequence, target, num_hidden=3, activation="dice", batch_norm=True,
            dropout_rate=0.1, cell_type="AGRU", dtype=torch.float64):
    """rankops.DIEN's eval forward from its state_dict `p`: (probability, logit, attention)."""
    p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in p.items()}
    cols = [v.to(dtype).reshape(-1, 1) for v in dense.values()]
    cols += [p[f"embeddings.{f}.weight"][category[f]] for f in CATEGORY if f in category]
    table = p["embeddings.feedid.weight"]
    e_target = table[target["feedid"]]
    state, att, _ = interest(e_target, table[sequence[SEQ_KEY]], sequence[f"{SEQ_KEY}_length"], model_weights(p),
                             cell_type, dtype)
    x = torch.cat(cols + [e_target, state], 1)
    i = 0
    for _ in range(num_hidden):
        x = x @ p[f"fcn.{i}.weight"].T + p[f"fcn.{i}.bias"]
        i += 1
        if activation == "dice":
            g = torch.sigmoid(_bn_eval(x, p, f"fcn.{i}.bn.", affine=False))
            x = p[f"fcn.{i}.alpha"] * (1 - g) * x + g * x
        else:
            x = torch.where(x >= 0, x, p[f"fcn.{i}.weight"] * x)
        i += 1
        if batch_norm:
            x = _bn_eval(x, p, f"fcn.{i}.", affine=True)
            i += 1
        if dropout_rate > 0:
            i += 1
    logit = x @ p["output_layer.weight"].T + p["output_layer.bias"]
    return torch.sigmoid(logit), logit, att


def draw_weights(H, nh, seed, amplitude=0.5):
    """Test weights: uniform(-amplitude, amplitude), gate biases 1 + that draw."""
    g = torch.Generator().manual_seed(seed)
    shapes = ((2 * nh, H + nh), (2 * nh,), (nh, H + nh), (nh,), (nh, H), (2 * nh, 2 * nh), (2 * nh,), (nh, 2 * nh),
              (nh,))
    ws = [((torch.rand(s, generator=g, dtype=torch.float64) * 2 - 1) * amplitude).float() for s in shapes]
    ws[1] += 1.0
    ws[6] += 1.0
    return ws
