"""Tiny seeded builds of the eight models for the sparse-gradient tests: B 33, vocabularies of
about 50 rows (so a batch repeats ids), T 5 for the sequence models, DIEN with and without the
auxiliary loss, BST with one and with two transformer blocks; `sparse` passes the sparse_grad keyword."""
import torch

import helpers as H
import rankops

B, T, T_NEG = 33, 5, 2
VOCAB = {"userid": 47, "feedid": 53, "device": 2, "authorid": 41, "bgm_song_id": 37, "bgm_singer_id": 43,
         "manual_tag_list": 23}
HIDDEN = [32, 16]
MODELS = ("dcn", "deepcrossing", "deepfm", "din", "afm", "bst", "bst2", "fwfm", "dien", "dien_aux")
NEG_KEY = "neg_his_read_comment_7d_seq"


def build(name, sparse, vocab=VOCAB, seed=42):
    """A CPU model in eval mode; the keyword is given only when set, so the dense twin is built
    exactly as before the keyword existed."""
    kw = {"sparse_grad": True} if sparse else {}
    torch.manual_seed(seed)
    if name == "dcn":
        m = rankops.DCNModel(None, hidden_units=HIDDEN, vocab_sizes=vocab, interaction_weights="frozen", **kw)
    elif name == "deepcrossing":
        m = rankops.DeepCrossingModel(None, residual_internal_dim=32, vocab_sizes=vocab,
                                      interaction_weights="frozen", **kw)
    elif name == "deepfm":
        m = rankops.DeepFM(None, embedding_dim=8, hidden_units=HIDDEN,
                           vocab_sizes={f: vocab[f] for f in rankops.deepfm.WECHAT_FIELDS}, **kw)
    elif name == "din":
        m = rankops.DIN(None, hidden_units=HIDDEN, vocab_sizes=vocab, interaction_weights="frozen", **kw)
    elif name == "afm":
        m = rankops.AFM(H.afm_feature_columns(vocab), 8, 16, **kw)
    elif name in ("bst", "bst2"):  # bst2: two transformer blocks, each with a position table of its own
        m = rankops.BSTModel(None, hidden_units=HIDDEN, vocab_sizes=vocab,
                             num_transformer_blocks=2 if name == "bst2" else 1, **kw)
    elif name == "fwfm":
        m = rankops.FwFM([vocab[f] for f in rankops.fwfm.FWFM_FIELDS], 8, **kw)
    elif name in ("dien", "dien_aux"):
        m = rankops.DIEN(None, hidden_units=HIDDEN, vocab_sizes=vocab, trainable=True,
                         use_auxiliary_loss=name == "dien_aux", negative_sample_number=T_NEG, **kw)
    else:
        raise ValueError(name)
    return H.randomize_eval_stats(m, seed + 1).eval()


def inputs(name, vocab=VOCAB, batch=B, seed=77):
    if name in ("dien", "dien_aux"):
        inp = H.din_inputs(batch, T, vocab, seed)
        if name == "dien_aux":
            g = torch.Generator().manual_seed(seed)
            inp["sequence"][NEG_KEY] = torch.randint(0, vocab["feedid"], (batch, (T - 1) * T_NEG), generator=g)
        return inp
    return H.make_inputs("bst" if name == "bst2" else name, {"vocab": vocab, "T": T}, batch, seed)


def labels(batch=B, seed=78):
    return (torch.rand(batch, generator=torch.Generator().manual_seed(seed)) < 0.3).float()


def loss_of(model, name, inp, label):
    """The scalar a train() loop of the model differentiates: BCE of the probability, plus DIN's l2
    term and DIEN's auxiliary loss where the model has one."""
    if name in ("dien", "dien_aux"):
        out = model(inp["dense"], inp["category"], inp["sequence"], inp["target"])
    else:
        out = H.as_tuple(H.call_model(model, "bst" if name == "bst2" else name, inp))
    loss = torch.nn.functional.binary_cross_entropy(out[0].reshape(-1), label)
    if name == "din":
        loss = loss + out[2]
    if name == "dien_aux":
        loss = loss + out[2]
    return loss


def is_table(model, param):
    return any(isinstance(m, torch.nn.Embedding) and m.weight is param for m in model.modules())
