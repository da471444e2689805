"""Speech marks from the phoneme alignment of the SoVITS engine (csrc/align.hip, SynthesizerTrn.last_alignment): pure host code.

A sentence's alignment counts frames of the 50-per-second pre-speed axis inside its span (`nf` of them); its audio is `n_samples`
samples at the model rate `sr`.  Phoneme j of sentence k runs from

    off_k + ends[j-1] / nf_k * n_samples_k / sr     to     off_k + ends[j] / nf_k * n_samples_k / sr,

off_k = sum over the sentences in front of k in OUTPUT order of (n_samples_i + gap) / sr.  This is exact for v1 / v2 at speed 1,
where n_samples_k = nf_k * prod(upsample_rates), and proportional for another speed_factor, for v3 / v4 (chunked flow matching and
SOLA) and under super-sampling.  Times are seconds, so an output sample rate, an encoding or a loudness gain does not move them.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np


def build_marks(sentences: Sequence[dict], sr: int, gap: int, order: Optional[Sequence[int]] = None, offset: float = 0.0) -> List[dict]:
    """`sentences[i]`: {"n_samples": emitted samples at the model rate `sr`; optional: "index" (default i), "text", "phones"
    (ids), "nf" (frames of the alignment span), "ends" (int [n_phones], exclusive end frame of each phoneme inside the span) and
    "score" (the alignment's mean log-probability), "word2ph" with "text" (phonemes per character: zh)}.  `gap`: the samples of
    silence after every sentence (int(sr * fragment_interval)); `order`: the output order as indices into `sentences` (default: as
    given); `offset`: where the first sentence starts.

    Returns one record per sentence in output order: {"index", "text", "start", "end", "confidence", "phones": [(phone_id, start,
    end), ...]}, and "units": [(char, start, end), ...] where word2ph is known.  Without "ends" (mode "sentence") "phones" is
    empty and "confidence" None; a fallback alignment (the search was not run: score -inf, possibly empty phonemes) keeps its
    -inf confidence.  The last record's end + gap / sr is the length of the audio."""
    if sr <= 0 or gap < 0:
        raise ValueError("build_marks: sr must be positive and gap non-negative")
    idx = list(range(len(sentences))) if order is None else [int(i) for i in order]
    if sorted(idx) != list(range(len(sentences))):
        raise ValueError("build_marks: order must be a permutation of the sentences")
    out, pos = [], 0          # pos: samples in front of the sentence (integers: the offsets do not drift)
    for i in idx:
        s = sentences[i]
        n = int(s["n_samples"])
        if n < 0:
            raise ValueError("build_marks: negative length")
        start, dur = offset + pos / sr, n / sr
        rec = {"index": int(s.get("index", i)), "text": s.get("text"), "start": start, "end": offset + (pos + n) / sr,
               "confidence": None, "phones": []}
        ends = s.get("ends")
        if ends is not None:
            ends = np.asarray(ends, np.int64)
            ids = list(s.get("phones", [None] * len(ends)))
            nf = int(s["nf"])
            if len(ids) != len(ends):
                raise ValueError(f"build_marks: sentence {i} has {len(ids)} phones and {len(ends)} ends")
            if len(ends) and (nf < 0 or ends[-1] > nf or np.any(np.diff(ends) < 0) or ends[0] < 0):
                raise ValueError(f"build_marks: the ends of sentence {i} are not non-decreasing frames of [0, {nf}]")
            score = s.get("score")
            rec["confidence"] = None if score is None else float(score)
            t = [start] + [start + (int(e) / nf) * dur if nf else start for e in ends]     # no frames: every phoneme is empty
            rec["phones"] = [(None if p is None else int(p), t[j], t[j + 1]) for j, p in enumerate(ids)]
            w2p = s.get("word2ph")
            if w2p is not None and s.get("text") is not None:
                w2p = [int(v) for v in w2p]
                if len(w2p) != len(s["text"]) or sum(w2p) != len(ends) or min(w2p, default=0) < 0:
                    raise ValueError(f"build_marks: word2ph of sentence {i} does not cover its text and phones")
                units, j = [], 0
                for ch, c in zip(s["text"], w2p):
                    units.append((ch, t[j], t[j + c]))     # a character without phonemes is an instant
                    j += c
                rec["units"] = units
        out.append(rec)
        pos += n + gap
    return out


def total_seconds(marks: Sequence[dict], sr: int, gap: int) -> float:
    """length of the audio the marks describe: the last sentence's end and its gap"""
    return (marks[-1]["end"] + gap / sr) if marks else 0.0


def to_json(marks: Sequence[dict]) -> list:
    """marks with tuples as lists and a -inf confidence as None, for json.dumps"""
    def conf(c):
        return None if c is None or not math.isfinite(c) else c
    out = []
    for m in marks:
        r = dict(m, confidence=conf(m["confidence"]), phones=[list(p) for p in m["phones"]])
        if "units" in m:
            r["units"] = [list(u) for u in m["units"]]
        out.append(r)
    return out
