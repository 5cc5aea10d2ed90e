"""The conversion step of the reference's demo (demo.ipynb cell 0): rhythm / pitch / timbre of one utterance replaced by
another speaker's, in the seven combinations R, F, U, RF, RU, FU, RFU.

Same inputs (two ``assets/demo.pkl``-style entries ``[speaker, emb f32[1,82], (mel[L,80], f0[L], L, uid)]``), same
padding / quantisation (``pad_seq_to_2`` to 192 frames, zero-padded F0 -> ``quantize_f0_numpy``), same F0 conversion
(``Generator_6`` logits -> argmax -> one-hot) and the same outputs ``[(name, mel[:len])]`` as the notebook.  What differs
is the schedule: the notebook runs seven batch-1 forwards, here the seven conditions are ONE batch-7 forward of the HIP
engine (every operator on the path is per-utterance, so the rows are the notebook's results).
The notebook's vocoder cell (WaveNet, external checkpoint) is out of scope; ``conversion_waveforms`` turns the mels into audio with the
checkpoint-free Griffin-Lim vocoder instead (vocoder.py).

``convert_batch`` is the same step for MANY pairs: every pair keeps its own ``conversion_frames()`` length and the forwards run as
ragged eval-mode batches (``lengths=``: every row comes out as if it had been run alone at its own length), sorted by length with
``plan_batches`` because a batch costs what its longest row costs.
"""
import numpy as np
import torch

from .utils import pad_seq_to_2, quantize_f0_numpy

CONDITIONS = ['R', 'F', 'U', 'RF', 'RU', 'FU', 'RFU']


def conversion_frames(lengths, max_len_pad=192):
    """Frames every utterance of one conversion is padded to.  The notebook's ``max_len_pad`` (192) when all of them fit, so
    short pairs give the notebook's results; otherwise the smallest multiple of 8 (the code down-sampling factor) that holds the
    longest: the batched Generator_3 call needs one T for both utterances, as the reference's does.  Frames beyond the engine's
    max_frames run in eval mode (Engine.reserve grows the workspace)."""
    longest = max(int(n) for n in lengths)
    return int(max_len_pad) if longest <= max_len_pad else -(-longest // 8) * 8


def _prepare(entry, max_len_pad, device):
    mel, f0, length, uid = entry[2]
    mel_pad, _ = pad_seq_to_2(mel[np.newaxis, :, :], max_len_pad)
    f0_pad = np.pad(f0, (0, max_len_pad - length), 'constant', constant_values=(0, 0))
    onehot = quantize_f0_numpy(f0_pad)[0][np.newaxis, :, :]
    return (torch.from_numpy(mel_pad.astype(np.float32)).to(device), torch.from_numpy(onehot.astype(np.float32)).to(device),
            torch.from_numpy(np.asarray(entry[1], np.float32)).to(device), int(length), uid)


def convert_f0(P, uttr_org_pad, f0_trg_onehot):
    """Generator_6 as F0 converter: logits -> argmax -> one-hot [1, T, 257]; also returns the class indices.  Both inputs are
    padded to one T (conversion_frames: any length, eval mode); a mismatch is refused."""
    if uttr_org_pad.shape[1] != f0_trg_onehot.shape[1]:
        raise ValueError('convert_f0: pad both utterances to conversion_frames() of their lengths '
                         f'(got {uttr_org_pad.shape[1]} and {f0_trg_onehot.shape[1]} frames)')
    with torch.no_grad():
        f0_pred = P(uttr_org_pad, f0_trg_onehot)[0]
        idx = f0_pred.argmax(dim=-1)
        onehot = torch.nn.functional.one_hot(idx, f0_pred.shape[-1]).to(f0_pred.dtype)[None]
    return onehot, idx


def demo_conversion(G, P, sbmt_i, sbmt_j, max_len_pad=192, device='cuda:0', conditions=CONDITIONS):
    """G: Generator_3, P: Generator_6 (both in eval mode, on `device`).  Returns [(name, mel ndarray[len, 80])].
    Both utterances are padded to conversion_frames(): max_len_pad when they fit, else one common multiple of 8."""
    T = conversion_frames((sbmt_i[2][2], sbmt_j[2][2]), max_len_pad)
    x_org, oh_org, emb_org, len_org, uid_org = _prepare(sbmt_i, T, device)
    x_trg, oh_trg, emb_trg, len_trg, _ = _prepare(sbmt_j, T, device)
    oh_con, _ = convert_f0(P, x_org, oh_trg)
    xf_org, xf_trg = torch.cat((x_org, oh_org), -1), torch.cat((x_org, oh_con), -1)
    x_f0 = torch.cat([xf_trg if 'F' in c else xf_org for c in conditions])
    x_rh = torch.cat([x_trg if 'R' in c else x_org for c in conditions])
    emb = torch.cat([emb_trg if 'U' in c else emb_org for c in conditions])
    with torch.no_grad():
        out = G(x_f0, x_rh, emb)
    res = []
    for n, c in enumerate(conditions):
        keep = len_trg if 'R' in c else len_org
        res.append(('{}_{}_{}_{}'.format(sbmt_i[0], sbmt_j[0], uid_org, c), out[n, :keep, :].cpu().numpy()))
    return res


def demo_conversion_codes(G, P, sbmt_i, sbmt_j, max_len_pad=192, device='cuda:0', conditions=CONDITIONS):
    """demo_conversion through the codes: the same names and shapes, from ONE batch-2 encode and one decode of the recombined codes
    instead of a forward (three encoders each) per condition.  In eval mode the content code depends on the mel columns alone, the pitch code
    on the one-hot columns alone and the rhythm code on x_org alone (reference model.py:194-229), so the seven conditions hold only these
    codes: row 0 of the encode is ([x_org | oh_org], x_org), row 1 is ([x_org | oh_con], x_trg)."""
    T = conversion_frames((sbmt_i[2][2], sbmt_j[2][2]), max_len_pad)
    x_org, oh_org, emb_org, len_org, uid_org = _prepare(sbmt_i, T, device)
    x_trg, oh_trg, emb_trg, len_trg, _ = _prepare(sbmt_j, T, device)
    oh_con, _ = convert_f0(P, x_org, oh_trg)
    with torch.no_grad():
        cx, cr, cf = G.encode(torch.cat((torch.cat((x_org, oh_org), -1), torch.cat((x_org, oh_con), -1))), torch.cat((x_org, x_trg)))
        rh = torch.tensor([1 if 'R' in c else 0 for c in conditions], device=cx.device)
        f0 = torch.tensor([1 if 'F' in c else 0 for c in conditions], device=cx.device)
        emb = torch.cat([emb_trg if 'U' in c else emb_org for c in conditions])
        out = G.decode(cx[:1].expand(len(conditions), -1, -1), cr[rh], cf[f0], emb)
    res = []
    for n, c in enumerate(conditions):
        keep = len_trg if 'R' in c else len_org
        res.append(('{}_{}_{}_{}'.format(sbmt_i[0], sbmt_j[0], uid_org, c), out[n, :keep, :].cpu().numpy()))
    return res


def convert_speakers(G, entry, embs, max_len_pad=192, device='cuda:0'):
    """One utterance decoded for every speaker row of embs [N, dim_spk_emb] from a SINGLE encode: entry is a demo.pkl-style
    ``[speaker, emb, (mel[L,80], f0[L], L, uid)]``; returns the mels as one device tensor [N, L, 80].  Row n equals
    ``G(x_f0, x_org, embs[n:n+1])[0, :L]`` of the padded utterance; the N - 1 repeated runs of the three encoders are what is saved."""
    T = conversion_frames((entry[2][2],), max_len_pad)
    x_org, oh_org, _, length, _ = _prepare(entry, T, device)
    embs = torch.as_tensor(embs, dtype=torch.float32).to(device)
    if embs.dim() != 2 or embs.shape[0] < 1:
        raise ValueError(f'convert_speakers: embs must be [N, dim_spk_emb] with N >= 1, got {tuple(embs.shape)}')
    N = embs.shape[0]
    with torch.no_grad():
        cx, cr, cf = G.encode(torch.cat((x_org, oh_org), -1), x_org)
        out = G.decode(cx.expand(N, -1, -1), cr.expand(N, -1, -1), cf.expand(N, -1, -1), embs)
    return out[:, :length]


def plan_batches(lengths, max_rows):
    """Batches for ragged forwards over utterances of the given lengths (host only): the indices sorted by length (ties in their given
    order) and cut into runs of at most max_rows.  Returns a list of index lists; every index appears exactly once, the batches come in
    non-decreasing order of their T, and a batch's T is its longest (= last) member's length."""
    max_rows = int(max_rows)
    if max_rows < 1:
        raise ValueError('plan_batches: max_rows must be at least 1')
    order = sorted(range(len(lengths)), key=lambda i: (int(lengths[i]), i))
    return [order[k:k + max_rows] for k in range(0, len(order), max_rows)]


def _pad_rows(rows, T):
    """[1, T_r, C] tensors -> [len(rows), T, C], zeros behind each row's own frames"""
    out = rows[0].new_zeros(len(rows), T, rows[0].shape[-1])
    for n, r in enumerate(rows):
        out[n, :r.shape[1]] = r[0]
    return out


def convert_batch(G, P, pairs, max_len_pad=192, max_rows=16, device='cuda:0', conditions=CONDITIONS):
    """demo_conversion for many pairs: pairs = [(sbmt_i, sbmt_j), ...] -> [demo_conversion(G, P, sbmt_i, sbmt_j, ...) per pair], the same
    names and shapes.  Every pair is padded to its OWN conversion_frames(); Generator_6 runs as ragged batches over the pairs and
    Generator_3 as ragged batches over pairs x conditions, both in plan_batches order with at most max_rows rows per forward."""
    prep = []
    for sbmt_i, sbmt_j in pairs:
        T = conversion_frames((sbmt_i[2][2], sbmt_j[2][2]), max_len_pad)
        prep.append((T, _prepare(sbmt_i, T, device), _prepare(sbmt_j, T, device)))
    # F0 conversion: one row per pair
    oh_con = [None] * len(pairs)
    with torch.no_grad():
        for batch in plan_batches([p[0] for p in prep], max_rows):
            lens = [prep[k][0] for k in batch]
            logits = P(_pad_rows([prep[k][1][0] for k in batch], lens[-1]), _pad_rows([prep[k][2][1] for k in batch], lens[-1]), lengths=lens)
            for n, k in enumerate(batch):
                lg = logits[n, :lens[n]]
                oh_con[k] = torch.nn.functional.one_hot(lg.argmax(dim=-1), lg.shape[-1]).to(lg.dtype)[None]
    # the conditions of every pair: one row each
    rows = []                                          # (pair, condition index, x_f0, x_rh, emb, T)
    for k, (T, (x_org, oh_org, emb_org, _, _), (x_trg, _, emb_trg, _, _)) in enumerate(prep):
        xf_org, xf_trg = torch.cat((x_org, oh_org), -1), torch.cat((x_org, oh_con[k]), -1)
        for n, c in enumerate(conditions):
            rows.append((k, n, xf_trg if 'F' in c else xf_org, x_trg if 'R' in c else x_org, emb_trg if 'U' in c else emb_org, T))
    res = [[None] * len(conditions) for _ in pairs]
    with torch.no_grad():
        for batch in plan_batches([r[5] for r in rows], max_rows):
            lens = [rows[i][5] for i in batch]
            out = G(_pad_rows([rows[i][2] for i in batch], lens[-1]), _pad_rows([rows[i][3] for i in batch], lens[-1]),
                    torch.cat([rows[i][4] for i in batch]), lengths=lens)
            for m, i in enumerate(batch):
                k, n = rows[i][0], rows[i][1]
                (sbmt_i, sbmt_j), c = pairs[k], conditions[n]
                keep = prep[k][2][3] if 'R' in c else prep[k][1][3]
                res[k][n] = ('{}_{}_{}_{}'.format(sbmt_i[0], sbmt_j[0], prep[k][1][4], c), out[m, :keep, :].cpu().numpy())
    return res


def adapt_speaker(G, entries, steps, lr=1e-4, train_decoder=True, emb0=None, max_rows=16, device='cuda:0'):
    """Adapt to a new speaker from a few of their utterances with the three encoders frozen: learn one speaker row (and, with
    train_decoder, fine-tune the decoder and the head) so that decoding each utterance's OWN codes with the row gives back its mel.

    entries: demo.pkl-style ``[speaker, emb f32[1,82], (mel[L,80], f0[L], L, uid)]``.  They are encoded ONCE, in eval mode, as ragged
    batches in plan_batches order (each at its own length rounded up to the code factors, at most max_rows per forward), and the codes and
    mels are zero-padded to one training shape [N, T] (T: the longest; it has to fit the engine's max_frames, N its batch).  Then `steps`
    fused decode steps run (Engine.g3_decode_train_step: decode, MSE, decoder backward, Adam over the decoder + head range from step 0
    and zeroed moments) -- no encoder forward, no encoder backward, no resampling draws.  The speaker row is updated by
    ``torch.optim.Adam(lr)`` from the step's per-row dc_trg summed over the batch; it starts at emb0 [1, dim_spk_emb], or at the mean of the
    entries' own rows.  train_decoder=False: the steps stop behind the backward (SS_STEP_NO_ADAM), so only the row learns and every model
    parameter keeps its bits.  Returns (row [1, dim_spk_emb] on the device, [loss of every step as float])."""
    hp = G.hparams_
    steps = int(steps)
    if not entries or steps < 0:
        raise ValueError('adapt_speaker: needs at least one entry and steps >= 0')
    f = int(np.lcm.reduce([hp.freq, hp.freq_2, hp.freq_3]))
    lens = [-(-int(e[2][2]) // f) * f for e in entries]
    N, T = len(entries), max(lens)
    prep = [_prepare(e, n, device) for e, n in zip(entries, lens)]
    was_training = G.training
    G.eval()
    try:
        G._ensure_engine(torch.device(device), N)
        eng = G._eng
        if T > eng.max_frames or N > eng.max_batch:
            raise ValueError(f'adapt_speaker: {N} utterances of up to {T} frames exceed the engine\'s training limits '
                             f'({eng.max_batch} x {eng.max_frames})')
        shp = eng.code_shapes(N, T)
        codes = {n: torch.zeros(shp[n], device=device) for n in ('x', 'r', 'f0')}
        with torch.no_grad():
            for batch in plan_batches(lens, max_rows):
                bl = [lens[k] for k in batch]
                x_org = _pad_rows([prep[k][0] for k in batch], bl[-1])
                x_f0 = torch.cat((x_org, _pad_rows([prep[k][1] for k in batch], bl[-1])), -1)
                for n, c in zip(('x', 'r', 'f0'), G.encode(x_f0, x_org, lengths=bl)):
                    codes[n][batch, :c.shape[1]] = c
        target = _pad_rows([p[0] for p in prep], T)
        row = torch.as_tensor(emb0, dtype=torch.float32).to(device).reshape(1, -1).clone() if emb0 is not None else torch.cat([p[2] for p in prep]).mean(0, keepdim=True)
        if row.shape[1] != hp.dim_spk_emb:
            raise ValueError(f'adapt_speaker: emb0 must hold dim_spk_emb = {hp.dim_spk_emb} values')
        row.requires_grad_(True)
        opt = torch.optim.Adam([row], lr=lr)
        if train_decoder:
            lo = eng.grad_split
            eng.adam_m[lo:].zero_()
            eng.adam_v[lo:].zero_()
            eng.set_adam(lr=lr, step=0)
        losses = []
        for _ in range(steps):
            loss, dc = eng.g3_decode_train_step(codes['x'], codes['r'], codes['f0'], row.detach().expand(N, -1), target,
                                                no_adam=not train_decoder, want_dc_trg=True)
            losses.append(loss.clone())
            row.grad = dc.sum(0, keepdim=True)
            opt.step()
    finally:
        G.train(was_training)
    return row.detach(), [float(v) for v in torch.cat(losses).cpu()] if losses else []


def conversion_waveforms(results, f0s=None, **kw):
    """demo_conversion's output ``[(name, mel[len, 80])]`` -> ``[(name, wav float64[256 (len - 1)])]`` at 16 kHz through the Griffin-Lim
    vocoder; convert_batch's output (one such list per pair) -> one such list per pair.  All the mels go through ONE vocoder.griffin_lim call
    (ragged batches of at most ``max_rows`` rows); keyword arguments are handed on to it.  ``f0s``: one F0 track per entry (ln Hz, -1e10
    unvoiced, as long as its mel; features.f0_from_norm makes one), nested as ``results`` is: the harmonic route of vocoder.griffin_lim."""
    from . import vocoder                               # vocoder imports plan_batches from here
    results = list(results)
    nested = bool(results) and isinstance(results[0], list)
    flat = [r for pair in results for r in pair] if nested else results
    if f0s is not None:
        f0s = list(f0s)
        if nested and (len(f0s) != len(results) or [len(p) for p in f0s] != [len(p) for p in results]):
            raise ValueError('conversion_waveforms: f0s must hold one track per result, nested as results is')
        kw['f0'] = [t for pair in f0s for t in pair] if nested else f0s
        if len(kw['f0']) != len(flat):
            raise ValueError('conversion_waveforms: f0s must hold one track per result, nested as results is')
    wavs = vocoder.griffin_lim([mel for _, mel in flat], **kw)
    out = [(name, wav) for (name, _), wav in zip(flat, wavs)]
    if not nested:
        return out
    it = iter(out)
    return [[next(it) for _ in pair] for pair in results]


def conversion_scores(results, targets, **kw):
    """demo_conversion's output ``[(name, mel[len, 80])]`` and one target mel per entry -> ``[(name, score dict)]``: the mel-cepstral
    distortion of each converted mel against its target along a DTW path (metrics.mcd_dtw; with ``f0x=`` / ``f0y=`` tracks, flat in the same
    order, also the F0 and voicing error).  convert_batch's output (one such list per pair) with targets nested the same way -> one such
    list per pair.  All the mels go through ONE metrics.mcd_dtw call; keyword arguments are handed on to it."""
    from . import metrics                               # metrics imports plan_batches from here
    results, targets = list(results), list(targets)
    nested = bool(results) and isinstance(results[0], list)
    flat = [r for pair in results for r in pair] if nested else results
    flat_t = [t for pair in targets for t in pair] if nested else targets
    if len(flat_t) != len(flat) or (nested and [len(p) for p in targets] != [len(p) for p in results]):
        raise ValueError('conversion_scores: targets must hold one mel per result, nested as results is')
    scores = metrics.mcd_dtw([mel for _, mel in flat], flat_t, **kw)
    out = [(name, s) for (name, _), s in zip(flat, scores)]
    if not nested:
        return out
    it = iter(out)
    return [[next(it) for _ in pair] for pair in results]


def conversion_stoi(waveforms, references, **kw):
    """conversion_waveforms' output ``[(name, wav)]`` and one reference waveform per entry -> ``[(name, score dict)]``: STOI (with
    ``extended=True`` ESTOI) of each waveform against its reference (metrics.stoi); nested input (one such list per pair) with references
    nested the same way -> one such list per pair.  All the waveforms go through ONE metrics.stoi call; keyword arguments are handed on to
    it.  STOI compares sample with sample, so it is defined only where the two are time-aligned: the conditions that keep the rhythm
    (``F``, ``U``, ``FU``) against their source recording, and any vocoded mel against the recording the mel came from (the vocoder trims
    exactly its 512 samples of padding, so sample 0 is sample 0).  A condition that converts rhythm (``R``, ``RF``, ``RU``, ``RFU``)
    changes the timing by construction and has no defined STOI; this function does not know the conditions' meaning and scores what it is
    given."""
    from . import metrics                               # metrics imports plan_batches from here
    waveforms, references = list(waveforms), list(references)
    nested = bool(waveforms) and isinstance(waveforms[0], list)
    flat = [w for pair in waveforms for w in pair] if nested else waveforms
    flat_r = [r for pair in references for r in pair] if nested else references
    if len(flat_r) != len(flat) or (nested and [len(p) for p in references] != [len(p) for p in waveforms]):
        raise ValueError('conversion_stoi: references must hold one waveform per entry, nested as waveforms is')
    scores = metrics.stoi(flat_r, [wav for _, wav in flat], **kw)
    out = [(name, s) for (name, _), s in zip(flat, scores)]
    if not nested:
        return out
    it = iter(out)
    return [[next(it) for _ in pair] for pair in waveforms]
