#!/usr/bin/env python3
"""Measured accuracy of the GPU vocoder against the fp64 restatement (tests/audio_ref.py) on the ragged batch of
tests/test_gpu_vocoder.py: per n_iter and utterance, the spectral convergence of both, the magnitude-spectrogram and wav relative
L2, and the wav2mel max abs error.  The gates of test_gpu_vocoder.py are min(cap, 2 x the worst value here).  Writes JSON to argv[1]."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "few-shot-transformer-tts_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import audio_ref as A  # noqa: E402
import test_gpu_vocoder as G  # noqa: E402


def main():
    from b2s_hip import vocoder
    G.fresh_hp()
    wavs = [G._signal(200 * (T - 1), 11 + i) for i, T in enumerate(G.TS)]
    mels = [A.get_spectrograms(w) for w in wavs]
    pad = np.zeros((len(G.TS), max(G.TS), 80), np.float32)
    for i, m in enumerate(mels):
        pad[i, :m.shape[0]] = m
    b = {"wavs": wavs, "mels": mels, "pad": pad}
    res = {"T": G.TS, "n_iter": {}}
    for n_iter in (0, 1, 5, 60):
        got = G.gpu_batch(b, n_iter)
        rows = []
        for i, T in enumerate(G.TS):
            wav_r, y_r, S = G.oracle(b, n_iter)[i]
            y_g = G.pre(got[i])
            sc_g, sc_r = A.spectral_convergence(y_g, S), A.spectral_convergence(y_r, S)
            rows.append({"T": T, "sc_gpu": sc_g, "sc_ref": sc_r, "sc_rel_diff": abs(sc_g - sc_r) / sc_r,
                         "mag_rel_l2": G.rel(np.abs(A.stft(y_g)), np.abs(A.stft(y_r))), "wav_rel_l2": G.rel(got[i], wav_r)})
        res["n_iter"][str(n_iter)] = rows
        print(n_iter, json.dumps({k: max(r[k] for r in rows) for k in ("sc_rel_diff", "mag_rel_l2", "wav_rel_l2")}), flush=True)
    wl = [len(w) for w in b["wavs"]]
    pad = np.zeros((len(wl), max(wl)), np.float32)
    for i, w in enumerate(b["wavs"]):
        pad[i, :len(w)] = w
    mels, frames = vocoder.wav2mel_batch(torch.from_numpy(pad).cuda(), wl)
    m = mels.cpu().numpy()
    res["wav2mel_max_abs"] = max(float(np.abs(m[i, :frames[i]] - A.get_spectrograms(w)).max()) for i, w in enumerate(b["wavs"]))
    print("wav2mel max abs", res["wav2mel_max_abs"])
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
