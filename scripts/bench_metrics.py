"""BLEU and ROUGE-L rewards beside CIDEr-D, at the shape of scripts/bench_cider.py: B 64 images, S 5 captions each, T 30, R 5 references
of up to Tr 30 tokens, V 10 000, the idf table of a corpus of 20 000 synthetic images; events around whole calls, warm-up calls
first, the routes alternating in one loop, medians:
  (a) dic_bleu, dic_rouge_l and dic_cider_d, each alone (native.bleu, native.rouge_l, cider.CiderD.score);
  (b) the host routes a user has without them: ids .cpu(), the fp64 restatement in Python (tests/metrics_common.py: dictionaries
      over id tuples / the O(n m) table, the references' tokens precomputed), the scores back to the device;
  (c) scst.scst_step with the CIDEr-D + BLEU-4 mix as reward_fn: metrics.reward_fn on the device, and the same mix through the
      host routes (tests/cider_common.py's restatement for the CIDEr-D part, as scripts/bench_cider.py has it).
usage: python scripts/bench_metrics.py [--batch 64] [--samples 5] [--steps 30] [--refs 5] [--vocab 10000] [--corpus 20000]
                                       [--iters 30] [--warmup 3] [--out profiles/metrics_bench.json]
Prints one line per route, the largest differences between (a) and (b) and a final JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from depth_image_captioning_pub_amd import cider, metrics, native, synthetic as syn
from depth_image_captioning_pub_amd.Captioning_models import scst
from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model.depth_models import CD_RNNDecoderWithSoftAttention
from tests import cider_common as cc
from tests import metrics_common as mc

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--samples", type=int, default=5)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--refs", type=int, default=5)
ap.add_argument("--vocab", type=int, default=10000)
ap.add_argument("--corpus", type=int, default=20000)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default="profiles/metrics_bench.json")
a = ap.parse_args()
B, S, T, R, V, dev = a.batch, a.samples, a.steps, a.refs, a.vocab, "cuda:0"
tok = syn.special_token_ids(V)
END = tok["<end>"]
W_BLEU4 = 0.5                                                                     # the mix: CIDEr-D + 0.5 BLEU-4

# the corpus: the batch is its first B images; references of 8 .. T - 1 words (+ <end> = at most Tr = T tokens)
corpus = syn.reference_captions(a.corpus, V, seed=31, n_refs=R, min_len=8, max_len=T - 1)
scorer = cider.CiderD.from_references(corpus, V, END, count_end=True, device=dev)
ref_ids, ref_counts = scorer.pack_references(corpus[:B])
Tr = int(ref_ids.shape[2])
# hypotheses for (a) / (b): captions of the corpus' own distribution (other images' references), <end>, then <end> padding
hyp = torch.full((B, S, T), END, dtype=torch.int64)
for b in range(B):
    for s in range(S):
        c = corpus[B + b * S + s][s % R][:T - 1]
        hyp[b, s, :len(c)] = torch.tensor(c)
hyp = hyp.to(dev)

table = dict(zip(scorer.idf_keys.tolist(), scorer.idf_vals.tolist()))
unseen = float(np.float32(scorer.idf_unseen))
ref_tokens = [[cc.caption_tokens(row, END, 1, V) for row in ref_ids[b, :int(ref_counts[b])].tolist()] for b in range(B)]
ref_vectors = [[cc.caption_vector(t, table, unseen, float) for t in ref_tokens[b]] for b in range(B)]


def _host(ids, score):
    rows = ids.cpu().tolist()                                                     # the copy synchronises the stream
    out = np.zeros((len(rows), len(rows[0])), dtype=np.float32)
    for b, caps in enumerate(rows):
        for s, row in enumerate(caps):
            out[b, s] = score(b, cc.caption_tokens(row, END, 1, V))
    return torch.from_numpy(out).to(ids.device)


def _host_bleu4(b, tokens):
    return mc.bleu_scores(mc.bleu_stats(tokens, ref_tokens[b]), float)[3]


def _host_rouge(b, tokens):
    return mc.rouge_score(tokens, ref_tokens[b], mc.BETA, float)[0]


def _host_cider(b, tokens):
    h = cc.caption_vector(tokens, table, unseen, float)
    return 10.0 / (4.0 * len(ref_vectors[b])) * sum(cc.similarity(h, r, 6.0, float)[0] for r in ref_vectors[b])


def host_mix(ids, lengths=None):
    return _host(ids, lambda b, t: _host_cider(b, t) + W_BLEU4 * _host_bleu4(b, t))


device_mix = metrics.reward_fn(ref_ids, ref_counts, id_end=END, vocab=V, count_end=True, cider=scorer,
                               weights={"CIDEr": 1.0, "Bleu_4": W_BLEU4})
w = syn.decoder_weights(V, seed=21)
dec = CD_RNNDecoderWithSoftAttention(128, 128, 2048, 128, V, 0.5)
dec.load_state_dict(w)
dec = dec.to(dev).eval()
opt = torch.optim.Adam(dec.parameters(), lr=1e-5)
fr, fd = syn.features(B, 22).to(dev), syn.features(B, 23, scale=0.5).to(dev)
step_seed = [0]


def step_with(reward):
    def run():
        step_seed[0] += 1
        return scst.scst_step(dec, opt, fr, fd, tok, reward, n_samples=S, max_length=T, seed=step_seed[0])
    return run


routes = (("bleu", lambda: native.bleu(hyp, ref_ids, ref_counts, END, V, True)),
          ("rouge_l", lambda: native.rouge_l(hyp, ref_ids, ref_counts, END, V, True)),
          ("cider_d", lambda: scorer.score(hyp, ref_ids, ref_counts)),
          ("host_bleu", lambda: _host(hyp, _host_bleu4)), ("host_rouge_l", lambda: _host(hyp, _host_rouge)),
          ("scst_step_device_mix", step_with(device_mix)), ("scst_step_host_mix", step_with(host_mix)))
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
times = {k: [] for k, _ in routes}
for it in range(a.iters + a.warmup):
    for key, fn in routes:
        torch.cuda.synchronize()
        ev[0].record()
        res = fn()
        ev[1].record()
        torch.cuda.synchronize()
        del res
        if it >= a.warmup:
            times[key].append(ev[0].elapsed_time(ev[1]))
out = {"B": B, "S": S, "T": T, "R": R, "Tr": Tr, "V": V, "corpus_images": a.corpus, "n_keys": int(scorer.idf_keys.numel()),
       "iters": a.iters, "warmup": a.warmup, "mix": f"CIDEr-D + {W_BLEU4} BLEU-4"}
for key, _ in routes:
    out[f"{key}_ms_median"] = statistics.median(times[key])
    out[f"{key}_ms_min"] = min(times[key])
out["bleu_over_cider_d"] = out["bleu_ms_median"] / out["cider_d_ms_median"]
out["rouge_l_over_cider_d"] = out["rouge_l_ms_median"] / out["cider_d_ms_median"]
got_b, got_r = native.bleu(hyp, ref_ids, ref_counts, END, V, True)[0][..., 3], native.rouge_l(hyp, ref_ids, ref_counts, END, V, True)
want_b, want_r = _host(hyp, _host_bleu4), _host(hyp, _host_rouge)
out["max_abs_diff_bleu4_device_host"] = float((got_b - want_b).abs().max())
out["max_abs_diff_rouge_l_device_host"] = float((got_r - want_r).abs().max())
out["max_abs_diff_mix_device_host"] = float((device_mix(hyp) - host_mix(hyp)).abs().max())
out["mean_bleu4"], out["mean_rouge_l"] = float(want_b.mean()), float(want_r.mean())
for key, _ in routes:
    print(f"{key}: median {out[f'{key}_ms_median']:.3f} ms, min {out[f'{key}_ms_min']:.3f} ms", flush=True)
print(f"dic_bleu / dic_cider_d = {out['bleu_over_cider_d']:.3f}, dic_rouge_l / dic_cider_d = {out['rouge_l_over_cider_d']:.3f}; "
      f"|device - host| <= {out['max_abs_diff_bleu4_device_host']:.2e} (BLEU-4, mean {out['mean_bleu4']:.2e}), "
      f"{out['max_abs_diff_rouge_l_device_host']:.2e} (ROUGE-L, mean {out['mean_rouge_l']:.3f}), "
      f"{out['max_abs_diff_mix_device_host']:.2e} (the mix)")
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
