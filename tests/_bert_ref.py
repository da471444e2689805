"""Plain torch fp32 mirror of what BertFeature computes: BERT's embeddings and the first `layers` post-LN encoder layers of a
transformers.BertModel state dict, one text at a time, [CLS] / [SEP] dropped (hidden_states[-3] of the 24-layer model at
layers = 22).  The reference of the packed-pass tests; test_bert_batch_gpu.py pins it against tests/golden/bert_large.npz."""
import torch
import torch.nn.functional as F


def tokenize(vocab, text):
    tok = {t: i for i, t in enumerate(vocab)}
    return [tok["[CLS]"]] + [tok.get(ch.lower(), tok["[UNK]"]) for ch in text] + [tok["[SEP]"]]


@torch.no_grad()
def bert_features(sd, vocab, text, layers=22, heads=16, eps=1e-12):
    sd = {k: v.float() for k, v in sd.items()}
    ids = torch.tensor(tokenize(vocab, text))
    T = ids.numel()
    x = sd["embeddings.word_embeddings.weight"][ids] + sd["embeddings.position_embeddings.weight"][:T] + \
        sd["embeddings.token_type_embeddings.weight"][0]
    h = x.shape[1]
    x = F.layer_norm(x, (h,), sd["embeddings.LayerNorm.weight"], sd["embeddings.LayerNorm.bias"], eps)
    for i in range(layers):
        p = f"encoder.layer.{i}."
        q, k, v = (F.linear(x, sd[p + f"attention.self.{n}.weight"], sd[p + f"attention.self.{n}.bias"])
                   .view(T, heads, h // heads).transpose(0, 1) for n in ("query", "key", "value"))
        a = torch.softmax(q @ k.transpose(1, 2) / (h // heads) ** 0.5, -1) @ v
        a = a.transpose(0, 1).reshape(T, h)
        o = F.linear(a, sd[p + "attention.output.dense.weight"], sd[p + "attention.output.dense.bias"]) + x
        x = F.layer_norm(o, (h,), sd[p + "attention.output.LayerNorm.weight"], sd[p + "attention.output.LayerNorm.bias"], eps)
        f = F.gelu(F.linear(x, sd[p + "intermediate.dense.weight"], sd[p + "intermediate.dense.bias"]))
        f = F.linear(f, sd[p + "output.dense.weight"], sd[p + "output.dense.bias"]) + x
        x = F.layer_norm(f, (h,), sd[p + "output.LayerNorm.weight"], sd[p + "output.LayerNorm.bias"], eps)
    return x[1:-1]
