"""Greedy-decode evaluation loop with the reference's entry point Cdepth_evaluation(atten, useData)
(depth_evaluation.py:26-193): for every trained parameter triple, load the three state_dicts into the drop-in modules,
switch everything to eval mode, and for each validation batch run  dpt -> standardize -> Resize(224) -> depth_encoder,
encoder, decoder.batch_sample  (depth_evaluation.py:146-165), then turn the token ids into captions up to '<end>'
(:167-176).  Every tensor operation runs in libdic_hip.so; the decode keeps the previous token on the device (the reference
copies it to the host every step, depth_models.py:298-299).

Out of scope here as in SURVEY.md section 2: the COCO dataset / annotation files and pycocoevalcap's METEOR scorer (a Java jar and
WordNet, evaluate_metrix.py:29) - `useData` must be "synthetic" (procedural images, a procedural vocabulary); the hypotheses
are returned and written next to the checkpoints.  CIDEr (evaluate_metrix.py:31) and, with it, Bleu_1..4 and ROUGE_L
(evaluate_metrix.py:28,30) are computed on request, on the device, over token ids against procedural reference captions
(cider.CiderD; metrics.evaluation_scores)."""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional

import numpy as np
import torch

from . import metrics as metrics_mod
from . import synthetic as syn
from ._lib import DicError
from .cider import CiderD
from .Captioning_models import constrained, util
from .Captioning_models import diverse as diverse_mod
from .Captioning_models import ensemble as ensemble_mod
from .Captioning_models.Base_caption_model.base_caption_models import CNNEncoder_Atten
from .Captioning_models.config import ConfigTrain
from .Captioning_models.Depth_caption_model.depth_models import (CD_RNNDecoderWithHardAttention,
                                                                 CD_RNNDecoderWithSoftAttention, Depth_CNN_endoder)
from .Captioning_models.Depth_caption_model.DPT_model import DPT_Depthestimator


def synthetic_vocabulary(vocab_size: int):
    """word <-> id dictionaries with the notebook's layout: ordinary words first, then <start>, <end>, <unk>, <null>
    (dataset/vocabulary_dict.ipynb cell 1)."""
    words = [f"w{i}" for i in range(vocab_size - 4)] + ["<start>", "<end>", "<unk>", "<null>"]
    return {w: i for i, w in enumerate(words)}, dict(enumerate(words))


def ids_to_captions(hypos_id: np.ndarray, id_to_word: Dict[int, str]) -> List[str]:
    """depth_evaluation.py:167-176: words up to (not including) the first '<end>'."""
    out = []
    for ids in hypos_id:
        line = []
        for i in ids:
            w = id_to_word[int(i)]
            if w == "<end>":
                break
            line.append(w)
        out.append(" ".join(line))
    return out


def _ensemble_entry(config, save_directory, param_files, dpt, n_batches, word_to_id, id_to_word, beam_size, length_penalty,
                    combine, limits, want_references, scores):
    """The "ensemble" entry of Cdepth_evaluation: every triple of param_files loaded into modules of its own, each batch decoded
    once by one beam over all of them (the batches, their seeds and references are the per-run loop's)."""
    dev = config.device
    members = []
    for f_enc, f_dec, f_denc in param_files.values():
        encoder = CNNEncoder_Atten(config.enc_img_size)
        decoder = CD_RNNDecoderWithSoftAttention(config.dim_attention, config.dim_embedding, config.dim_encoder, config.dim_hidden,
                                                 config.vocab_size)
        depth_encoder = Depth_CNN_endoder(config.enc_img_size)
        for m, f in ((encoder, f_enc), (decoder, f_dec), (depth_encoder, f_denc)):
            m.load_state_dict(torch.load(f"{save_directory}/{f}", weights_only=True))
            m.to(dev)
            m.eval()
        members.append((encoder, decoder, depth_encoder))
    hypos_id, references = [], []
    for b in range(n_batches):
        raw = syn.raw_images(config.batch_size, seed=5000 + b).to(dev)
        imgs, imgs_for_dep = util.device_transforms(raw)
        depth_maps = dpt.depth_maps_for_training(imgs_for_dep)
        if want_references:
            references += syn.reference_captions(config.batch_size, config.vocab_size, seed=5000 + b)
        hypos_id.append(ensemble_mod.ensemble_beam_sample([d for _, d, _ in members], [e(imgs) for e, _, _ in members],
                                                          [de(depth_maps) for _, _, de in members], word_to_id,
                                                          beam_size=beam_size, length_penalty=length_penalty, combine=combine,
                                                          **limits))
    hypos_id = np.concatenate(hypos_id)
    entry = {"hypotheses": ids_to_captions(hypos_id, id_to_word), "ids": hypos_id}
    entry.update(scores(hypos_id, references))
    return entry


@torch.no_grad()
def Cdepth_evaluation(atten: str, useData: str, config=None, param_files: Optional[Dict[str, List[str]]] = None,
                      n_batches: int = 2, dpt: Optional[DPT_Depthestimator] = None, beam_size: int = 1,
                      length_penalty: float = 0.0, n_samples: int = 0, temperature: float = 1.0, top_k: int = 0,
                      top_p: float = 1.0, seed: int = 0, cider: bool = False, metrics: bool = False, suppress=None,
                      min_length: int = 0, no_repeat_ngram: int = 0, beam_groups: int = 1, diversity: float = 0.0,
                      ensemble: bool = False, ensemble_combine: str = "prob", attention_seed: Optional[int] = None):
    """Returns {key: {"hypotheses": [...], "ids": np.int64 [N,30]}} per parameter triple.  `param_files` maps a key to
    [encoder, decoder, depth-encoder] checkpoint file names inside the run's save directory (config.depth_*_parameter_files
    in the reference, config.py:131-136); default = the best-validation files train_Cdepth_* wrote for run 0.
    beam_size > 1 (soft attention only) decodes with decoder.beam_sample - the best of `beam_size` hypotheses per image, ranked
    by score / length^length_penalty - instead of the reference's greedy batch_sample; 1 is the greedy loop itself.
    n_samples > 0 (soft attention only) ADDS to each result "samples", a list of `n_samples` caption strings per image drawn with
    decoder.stochastic_sample(temperature, top_k, top_p), and "sample_ids" np.int64 [N,n_samples,30]; batch b is seeded with
    seed + b.  The hypotheses, the ids and the written file do not depend on it.
    attention_seed (atten="hard" only): with it a hard model decodes CONDITIONAL on attention noise drawn from a seed - beam_size > 1
    with decoder.hard_beam_sample (noise shared by an image's hypotheses), n_samples > 0 with decoder.hard_stochastic_sample
    (noise per row); batch b is seeded attention_seed + b.  None (default): both refuse for a hard model as before; the greedy
    path of a hard model never uses it.
    cider=True ADDS "CIDEr": the mean CIDEr-D (evaluate_metrix.py:31; x10 as pycocoevalcap reports it) of the hypotheses against
    synthetic.reference_captions(batch_size, vocab_size, seed=5000 + b) of batch b, five per image, scored on the device as decoded
    strings are (count_end=False); the idf table is that of all the evaluated images' references.  Nothing else depends on it.
    metrics=True ADDS the reference's report without METEOR - "Bleu_1" .. "Bleu_4" (corpus BLEU), "ROUGE_L" (mean over the images)
    and "CIDEr" (as cider=True) - over the same references, by metrics.evaluation_scores.  Nothing else depends on it.
    suppress (a sequence of words or token ids, e.g. ("<start>", "<unk>", "<null>")), min_length, no_repeat_ngram: constrained
    decoding (Captioning_models/constrained.py).  With the defaults (None, 0, 0) the loop, its results and the
    written file are what they were without these keywords.  With any of them set the hypotheses come from the constrained beam
    search - no suppressed token, no '<end>' before `min_length` words, no n-gram of `no_repeat_ngram` tokens twice; beam_size=1 is
    then constrained greedy decoding - and, when n_samples > 0, the samples from the constrained sampler.  A hard model needs
    attention_seed for either.
    ensemble=True (atten="soft" only) ADDS the key "ensemble" to the result and to the written file: all triples of `param_files`
    are loaded side by side and every batch is decoded ONCE by ensemble.ensemble_beam_sample over all of them - one beam over the
    members' combined word distribution (ensemble_combine "prob": averaged probabilities, "logprob": averaged log-probabilities;
    uniform weights) - with the loop's beam_size (1: ensemble greedy), length_penalty and constraints.  Its entry
    holds "hypotheses", "ids" and the metrics / CIDEr figures when requested.  The per-run entries do not depend on it; a run key
    named "ensemble" is refused.
    beam_groups > 1: diverse beam search (Captioning_models/diverse.py) - the beam_size beams are beam_groups groups
    (beam_groups must divide beam_size) that pay `diversity` for repeating an earlier group's token of the step.  The run's
    hypothesis is the group winner with the highest ranking value score / length^length_penalty, ties to the lower group; the entry
    gains "group_hypotheses", the beam_groups winners of every image in group order, and "group_ids" np.int64 [N,beam_groups,30],
    and the group winners are also written to `<useData>_group_hypotheses.json`.  The constraints apply as above.  Refused with
    beam_size == 1, with n_samples > 0 and with ensemble=True.  With the defaults (1, 0.0) nothing changes."""
    if useData != "synthetic":
        raise DicError(f"useData={useData!r}: MSCOCO and the original dataset are not available offline; use 'synthetic'")
    if atten not in ("soft", "hard"):
        raise DicError("atten must be 'soft' or 'hard'")
    if int(beam_size) < 1:
        raise DicError(f"beam_size={beam_size!r} must be at least 1")
    if attention_seed is not None and atten != "hard":
        raise DicError("attention_seed seeds the attention noise of the hard-attention decoder: it needs atten='hard'")
    if int(beam_size) > 1 and atten != "soft" and attention_seed is None:
        raise DicError("beam_size > 1 needs atten='soft': beam search is built for the soft-attention decoder only (a hard model "
                       "searches conditional on its attention noise when attention_seed is given)")
    if int(n_samples) < 0:
        raise DicError(f"n_samples={n_samples!r} must be at least 0")
    if int(n_samples) > 0 and atten != "soft" and attention_seed is None:
        raise DicError("n_samples > 0 needs atten='soft': sampling is built for the soft-attention decoder only (a hard model "
                       "samples conditional on its attention noise when attention_seed is given)")
    if int(beam_groups) < 1:
        raise DicError(f"beam_groups={beam_groups!r} must be at least 1")
    if int(beam_groups) > 1:
        if int(beam_size) == 1:
            raise DicError("beam_groups > 1 needs beam_size > 1: the groups divide the beams of a beam search")
        if int(n_samples) > 0:
            raise DicError("beam_groups > 1 cannot be combined with n_samples > 0: take the variety from one of the two")
        if ensemble:
            raise DicError("beam_groups > 1 cannot be combined with ensemble=True: the ensemble route has no diverse form")
        diverse_mod.check_groups("Cdepth_evaluation", beam_size, beam_groups, diversity)
    constrained.check_constraints("Cdepth_evaluation", min_length, no_repeat_ngram)
    constrain = bool(suppress is not None and len(suppress) > 0) or int(min_length) > 0 or int(no_repeat_ngram) > 0
    if constrain and atten == "hard" and attention_seed is None:
        raise DicError("suppress / min_length / no_repeat_ngram need attention_seed with atten='hard': the constrained routes of a "
                       "hard model decode conditional on its attention noise")
    if ensemble and atten != "soft":
        raise DicError("ensemble=True needs atten='soft': the ensemble beam search is built for the soft-attention decoders only")
    if ensemble and ensemble_combine not in ("prob", "logprob"):
        raise DicError(f"ensemble_combine must be 'prob' or 'logprob', got {ensemble_combine!r}")
    if ensemble and param_files is not None and "ensemble" in param_files:
        raise DicError("param_files has a run named 'ensemble': with ensemble=True that key holds the ensemble's result")
    config = config or ConfigTrain()
    dev = config.device
    tag = f"depth_{atten}"
    save_directory = config.save_directory_Cdep_soft if atten == "soft" else config.save_directory_Cdep_hard
    if param_files is None:
        param_files = {"run0": [f"{tag}_encoder_best_synthetic0.pth", f"{tag}_decoder_best_synthetic0.pth",
                                f"{tag}_D_encoder_best_synthetic0.pth"]}
    word_to_id, id_to_word = synthetic_vocabulary(config.vocab_size)
    if constrain:
        suppress = constrained.suppress_ids("Cdepth_evaluation", suppress, word_to_id)      # (an unknown word is refused before any work)
        limits = dict(suppress=suppress, min_length=int(min_length), no_repeat_ngram=int(no_repeat_ngram))
    encoder = CNNEncoder_Atten(config.enc_img_size)                                          # depth_evaluation.py:108-129
    if atten == "soft":
        decoder = CD_RNNDecoderWithSoftAttention(config.dim_attention, config.dim_embedding, config.dim_encoder,
                                                 config.dim_hidden, config.vocab_size)
    else:
        decoder = CD_RNNDecoderWithHardAttention(config.dim_attention, config.dim_embedding, config.dim_encoder,
                                                 config.dim_hidden, config.vocab_size, dev, config.dropout)
    depth_encoder = Depth_CNN_endoder(config.enc_img_size)
    dpt = dpt if dpt is not None else DPT_Depthestimator(getattr(config, "dpt_config", None))
    for m in (encoder, decoder, depth_encoder, dpt):
        m.to(dev)
        m.eval()                                                                            # :131-134

    def _scores(ids, refs):
        if metrics:
            return metrics_mod.evaluation_scores(torch.from_numpy(ids), refs, config.vocab_size, word_to_id["<end>"], dev)
        if cider:
            scorer = CiderD.from_references(refs, config.vocab_size, word_to_id["<end>"], count_end=False, device=dev)
            ref_ids, ref_counts = scorer.pack_references(refs)
            return {"CIDEr": float(scorer.corpus_score(torch.from_numpy(ids).long().to(dev), ref_ids, ref_counts))}
        return {}

    results = {}
    for key, (f_enc, f_dec, f_denc) in param_files.items():
        encoder.load_state_dict(torch.load(f"{save_directory}/{f_enc}", weights_only=True))       # :139-144
        decoder.load_state_dict(torch.load(f"{save_directory}/{f_dec}", weights_only=True))
        depth_encoder.load_state_dict(torch.load(f"{save_directory}/{f_denc}", weights_only=True))
        hypos_id, sample_ids, group_ids = [], [], []
        references = []
        for b in range(n_batches):
            raw = syn.raw_images(config.batch_size, seed=5000 + b).to(dev)
            imgs, imgs_for_dep = util.device_transforms(raw)
            depth_maps = dpt.depth_maps_for_training(imgs_for_dep)                          # :155-159
            depth_features = depth_encoder(depth_maps)                                      # :161
            feature = encoder(imgs)                                                         # :164
            if cider or metrics:
                references += syn.reference_captions(config.batch_size, config.vocab_size, seed=5000 + b)
            if int(beam_groups) > 1:
                seeds = dict(attention_seed=int(attention_seed) + b) if atten == "hard" else {}
                kp = int(beam_size) // int(beam_groups)
                ids, scores, lengths = diverse_mod.diverse_beam_sample(
                    decoder, feature, depth_features, word_to_id, beam_size=int(beam_size), groups=int(beam_groups),
                    diversity=float(diversity), length_penalty=length_penalty, return_all=True,
                    **(limits if constrain else {}), **seeds)
                ids, scores, lengths = ids[:, ::kp], scores[:, ::kp].astype(np.float64), lengths[:, ::kp].astype(np.float64)
                value = scores / lengths ** float(length_penalty) if length_penalty else scores
                best = value.argmax(axis=1)                      # (the first maximum: ties go to the lower group)
                group_ids.append(ids)
                hypos_id.append(ids[np.arange(ids.shape[0]), best])
            elif constrain:
                seeds = dict(attention_seed=int(attention_seed) + b) if atten == "hard" else {}
                hypos_id.append(constrained.constrained_beam_sample(decoder, feature, depth_features, word_to_id,
                                                                    beam_size=int(beam_size), length_penalty=length_penalty,
                                                                    **limits, **seeds))
            elif int(beam_size) > 1 and atten == "hard":
                hypos_id.append(decoder.hard_beam_sample(feature, depth_features, word_to_id, beam_size=int(beam_size),
                                                         length_penalty=length_penalty, attention_seed=int(attention_seed) + b))
            elif int(beam_size) > 1:
                hypos_id.append(decoder.beam_sample(feature, depth_features, word_to_id, beam_size=int(beam_size),
                                                    length_penalty=length_penalty))
            else:
                hypos_id.append(decoder.batch_sample(feature, depth_features, word_to_id))     # :165
            if int(n_samples) > 0 and constrain:
                drawn = constrained.constrained_stochastic_sample(decoder, feature, depth_features, word_to_id,
                                                                  n_samples=int(n_samples), temperature=temperature, top_k=top_k,
                                                                  top_p=top_p, seed=int(seed) + b, **limits, **seeds)
                sample_ids.append(drawn.reshape(drawn.shape[0], int(n_samples), -1))
            elif int(n_samples) > 0 and atten == "hard":
                drawn = decoder.hard_stochastic_sample(feature, depth_features, word_to_id, n_samples=int(n_samples),
                                                       temperature=temperature, top_k=top_k, top_p=top_p, seed=int(seed) + b,
                                                       attention_seed=int(attention_seed) + b)
                sample_ids.append(drawn.reshape(drawn.shape[0], int(n_samples), -1))
            elif int(n_samples) > 0:
                drawn = decoder.stochastic_sample(feature, depth_features, word_to_id, n_samples=int(n_samples),
                                                  temperature=temperature, top_k=top_k, top_p=top_p, seed=int(seed) + b)
                sample_ids.append(drawn.reshape(drawn.shape[0], int(n_samples), -1))
        hypos_id = np.concatenate(hypos_id)
        hypos_word = ids_to_captions(hypos_id, id_to_word)
        results[key] = {"hypotheses": hypos_word, "ids": hypos_id}
        if int(n_samples) > 0:
            sample_ids = np.concatenate(sample_ids)
            results[key]["samples"] = [ids_to_captions(rows, id_to_word) for rows in sample_ids]
            results[key]["sample_ids"] = sample_ids
        if int(beam_groups) > 1:
            group_ids = np.concatenate(group_ids)
            results[key]["group_hypotheses"] = [ids_to_captions(rows, id_to_word) for rows in group_ids]
            results[key]["group_ids"] = group_ids
        # depth_evaluation.py:178-184 scores the hypotheses with pycocoevalcap: BLEU, ROUGE-L and CIDEr are computed here on request,
        # over token ids on the device; METEOR (a Java jar and WordNet) is out of scope.
        results[key].update(_scores(hypos_id, references))
    if ensemble:
        results["ensemble"] = _ensemble_entry(config, save_directory, param_files, dpt, n_batches, word_to_id, id_to_word,
                                              int(beam_size), length_penalty, ensemble_combine, limits if constrain else {},
                                              cider or metrics, _scores)
    with open(os.path.join(save_directory, f"{useData}_hypotheses.json"), "w") as f:
        json.dump({k: v["hypotheses"] for k, v in results.items()}, f)
    if int(beam_groups) > 1:
        with open(os.path.join(save_directory, f"{useData}_group_hypotheses.json"), "w") as f:
            json.dump({k: v["group_hypotheses"] for k, v in results.items()}, f)
    return results
