"""Thin Python owner of one HIP engine: allocates the four parameter arenas and the workspace as torch CUDA
tensors (PyTorch is only the allocator / stream provider here), hands their device pointers to the C ABI and
exposes zero-copy parameter / gradient views under the reference's state_dict names."""
import ctypes as C

import numpy as np
import torch

from . import _capi
from .hparams import check_hparams  # noqa: F401  (the host-side form of the refusals Engine() raises)

KIND ={'G3': 3, 'G6': 6, 'interp': 0}
RAGGED = ('ragged',)                   # Engine._fwd_bt after a forward over per-row lengths: there is no backward for it


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def step_flags(no_adam=False, split_backward=False, split_no_join=False, accumulate=False, bucket=False):
    """The SS_STEP_* word of the training-step entry points from keyword booleans."""
    return ((_capi.SS_STEP_NO_ADAM if no_adam else 0) | (_capi.SS_STEP_SPLIT_BACKWARD if split_backward else 0)
            | (_capi.SS_STEP_SPLIT_NO_JOIN if split_no_join else 0) | (_capi.SS_STEP_ACCUMULATE if accumulate else 0)
            | (_capi.SS_STEP_BUCKET if bucket else 0))


def draw_interp(batch, ncalls, hp, generator=None):
    """Draw the InterpLnr randomness exactly as the reference consumes it (model.py:392-393 then 399-402, per
    call, from the default CPU generator unless one is given).  Returns (scales f32[ncalls, B*S], len_seg i32[...])."""
    S = hp.max_len_seq // hp.min_len_seg + 1
    sc, ls = [], []
    for _ in range(ncalls):
        sc.append(torch.rand(batch * S, generator=generator) + 0.5)
        ls.append(torch.randint(low=hp.min_len_seg, high=hp.max_len_seg, size=(batch * S, 1), generator=generator))
    return torch.stack(sc), torch.stack(ls).reshape(ncalls, -1).to(torch.int32)


def check_lengths(lengths, B, T, factors=(1,), device=None):
    """Per-row lengths of a ragged eval-mode batch -> contiguous int32 tensor on `device` (the i32[B] array the ss_*_ragged entry points read).
    lengths: a host list / array / tensor, or a device int tensor.  What the host can see is validated here -- one length per row, each a
    multiple of every factor and within [largest factor, T] -- and a ValueError is raised before anything is enqueued; a tensor that already
    lives on a GPU is checked for its count only (reading it would synchronise), and the kernels clamp what they read to [0, T]."""
    t = lengths if isinstance(lengths, torch.Tensor) else torch.as_tensor(np.asarray(lengths))
    if t.dim() != 1 or t.numel() != B:
        raise ValueError(f'speechsplit_amd: lengths must hold one entry per row ({B}), got shape {tuple(t.shape)}')
    if t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError('speechsplit_amd: lengths must be integers')
    if not t.is_cuda:
        lo = max(int(f) for f in factors)
        for b, n in enumerate(t.tolist()):
            if any(n % int(f) for f in factors):
                raise ValueError(f'speechsplit_amd: lengths[{b}] = {n} is not a multiple of the code factors {tuple(int(f) for f in factors)}')
            if n < lo or n > T:
                raise ValueError(f'speechsplit_amd: lengths[{b}] = {n} is outside [{lo}, T = {T}]')
    return t.to(device=device if device is not None else t.device, dtype=torch.int32).contiguous()


class Engine:
    def __init__(self, kind, hp, max_batch, max_frames=None, device=None, alloc=None):
        """alloc(name, shape, dtype): optional provider of every device buffer the engine owns or returns -- the arenas 'params' / 'grads' /
        'adam_m' / 'adam_v' (zero-filled by the provider), the workspace 'ws' (uint8, 256-byte aligned, any contents), 'loss', and the
        outputs of the forwards and input-gradient backwards ('out', 'dx_f0', ...) -- for callers that place them themselves."""
        if not torch.cuda.is_available():
            raise RuntimeError('speechsplit_amd.Engine needs a ROCm GPU (no CPU fallback)')
        self.lib = _capi.lib()
        self.kind = kind
        self.hp = hp
        self.device = torch.device(device if device is not None else f'cuda:{torch.cuda.current_device()}')
        self.max_batch = int(max_batch)
        self.max_frames = int(max_frames or hp.max_len_pad)
        self._stagers = {}
        self._alloc = alloc
        self._fwd_bt = None                # (B, T) of the last g3_forward / g6_forward (RAGGED: it ran over lengths); None after any other forward
        self._hps = _capi.hparams_struct(hp)
        self.h = self.lib.ss_create(KIND[kind], C.byref(self._hps), self.max_batch, self.max_frames)
        if not self.h:
            raise RuntimeError('speechsplit_amd: ' + self.lib.ss_last_error().decode())
        self.table = []
        name = C.create_string_buffer(256)
        off, nd, shp = C.c_long(), C.c_int(), (C.c_long * 3)()
        for i in range(self.lib.ss_num_params(self.h)):
            _capi.check(self.lib.ss_param_info(self.h, i, name, 256, C.byref(off), C.byref(nd), C.byref(shp)))
            self.table.append((name.value.decode(), off.value, tuple(shp[k] for k in range(nd.value))))
        n = self.lib.ss_arena_numel(self.h)
        with torch.cuda.device(self.device):
            self.params = self._new('params', (n,), zero=True)
            self.grads = self._new('grads', (n,), zero=True)
            self.adam_m = self._new('adam_m', (n,), zero=True)
            self.adam_v = self._new('adam_v', (n,), zero=True)
            self.ws = self._new('ws', (self.lib.ss_workspace_bytes(self.h),), torch.uint8)
            self.loss = self._new('loss', (1,), zero=True)
            _capi.check(self.lib.ss_bind(self.h, _ptr(self.params), _ptr(self.grads), _ptr(self.adam_m), _ptr(self.adam_v),
                                         _ptr(self.ws), self.ws.numel(), _stream()))

    def _new(self, name, shape, dtype=torch.float32, zero=False):
        if self._alloc is not None:
            t = self._alloc(name, tuple(shape), dtype)
            assert t.is_contiguous() and tuple(t.shape) == tuple(shape) and t.dtype == dtype, name
            return t
        return (torch.zeros if zero else torch.empty)(tuple(shape), dtype=dtype, device=self.device)

    def __del__(self):
        try:
            if getattr(self, 'h', None):
                self.lib.ss_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ------------------------------------------------------------------ parameters
    def views(self, arena):
        return {n: arena[o:o + int(np.prod(s))].view(*s) for n, o, s in self.table}

    def param_views(self):
        return self.views(self.params)

    def grad_views(self):
        return self.views(self.grads)

    def load_weights(self, weights):
        """weights: dict name -> numpy / tensor with the reference's shapes."""
        pv = self.param_views()
        for n, _, s in self.table:
            w = weights[n]
            w = torch.from_numpy(np.ascontiguousarray(w)) if isinstance(w, np.ndarray) else w.detach()
            assert tuple(w.shape) == tuple(s), (n, w.shape, s)
            pv[n].copy_(w.to(torch.float32))

    def set_adam(self, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=0):
        _capi.check(self.lib.ss_set_adam(self.h, lr, beta1, beta2, eps, int(step), _stream()))

    # ------------------------------------------------------------------ workspace
    def plan_bytes(self, B, T):
        """Workspace bytes an eval-mode forward of shape (B, T) needs (ss_plan_bytes); raises for a shape the engine cannot run."""
        n = self.lib.ss_plan_bytes(self.h, int(B), int(T))
        if n < 0:
            raise RuntimeError('speechsplit_amd: ' + self.lib.ss_last_error().decode())
        return int(n)

    def reserve(self, B, T):
        """Make the workspace hold an eval-mode forward of (B, T): grow it through ss_set_workspace when the plan does not fit (the
        engine, its parameter arenas and the Adam state stay as they are), never shrink it.  Returns True when it grew."""
        need = self.plan_bytes(B, T)
        if need <= self.ws.numel():
            return False
        with torch.cuda.device(self.device):
            ws = self._new('ws', (need,), torch.uint8)
            _capi.check(self.lib.ss_set_workspace(self.h, _ptr(ws), ws.numel(), _stream()))
        self.ws = ws                                   # the call synchronised: nothing runs on the old workspace any more
        return True

    def _reserve_eval(self, B, T, training):
        if not training and T > self.max_frames:       # frames beyond max_frames: eval-mode forwards only (ss_plan_bytes)
            self.reserve(B, T)

    # ------------------------------------------------------------------ helpers
    def _f(self, t):
        return t.to(device=self.device, dtype=torch.float32).contiguous()

    def _i(self, t):
        return t.to(device=self.device, dtype=torch.int32).contiguous()

    def _draws(self, draws):
        """Device tensors pass through untouched; host draws go through a pinned ring with one non-blocking copy on the
        compute stream (staging.DrawStager) -- never a pageable, blocking `.to(device)`."""
        if draws is None:
            return None, None
        sc, ls = draws
        sc, ls = torch.as_tensor(sc), torch.as_tensor(ls)
        if sc.is_cuda and ls.is_cuda:
            return self._f(sc), self._i(ls)
        sc, ls = sc.reshape(sc.shape[0], -1), ls.reshape(ls.shape[0], -1)
        key = tuple(sc.shape)
        st = self._stagers.get(key)
        if st is None:
            from .staging import DrawStager
            st = self._stagers[key] = DrawStager(self.device, key[0], key[1])
        return st.stage(sc, ls)

    def _lengths(self, lengths, B, T, training=False):
        """lengths of a ragged eval-mode batch -> device i32[B] (check_lengths); ValueError for what the host can see is wrong, training included."""
        if training:
            raise ValueError('speechsplit_amd: lengths (a ragged batch) are for eval-mode forwards only, not training=True')
        hp = self.hp
        return check_lengths(lengths, B, T, (hp.freq, hp.freq_2, hp.freq_3), self.device)

    # ------------------------------------------------------------------ Generator_3
    def g3_forward(self, x_f0, x_org, c_trg, draws=None, training=False, lengths=None):
        """lengths (eval mode only): one frame count per row -- a ragged batch (ss_g3_forward_ragged).  Row b of the result equals the
        forward of that utterance alone at T = lengths[b]; the frames behind are zeros, the input frames behind are never read."""
        B, T, _ = x_org.shape
        ln = self._lengths(lengths, B, T, training) if lengths is not None else None
        x_f0, x_org, c_trg = self._f(x_f0), self._f(x_org), self._f(c_trg)
        if c_trg.shape[0] != B:
            c_trg = c_trg.expand(B, -1).contiguous()
        sc, ls = self._draws(draws)
        out = self._new('out', (B, T, self.hp.dim_freq))
        self._fwd_bt = None
        self._reserve_eval(B, T, training)
        if ln is not None:
            _capi.check(self.lib.ss_g3_forward_ragged(self.h, _ptr(x_f0), _ptr(x_org), _ptr(c_trg), _ptr(ln), B, T, 0, _ptr(out), _stream()))
            self._fwd_bt = RAGGED                      # eval-only: no input gradients, and ss_*_backward* refuses
            return out
        _capi.check(self.lib.ss_g3_forward(self.h, _ptr(x_f0), _ptr(x_org), _ptr(c_trg), _ptr(sc), _ptr(ls), B, T,
                                           int(training), _ptr(out), _stream()))
        self._fwd_bt = (B, T)
        return out

    G3_INPUTS = ('x_f0', 'x_org', 'c_trg')
    G6_INPUTS = ('x_org', 'f0_trg')

    def _input_grad_buffers(self, names, inputs):
        """Fresh dense outputs for the requested input gradients of the last forward, in the entry point's order (None: not asked for)."""
        unknown = set(inputs) - set(names)
        if unknown:
            raise ValueError(f'speechsplit_amd: no input named {sorted(unknown)} (expected some of {names})')
        if self._fwd_bt == RAGGED:
            raise RuntimeError('speechsplit_amd: backward: the last forward ran over per-row lengths (a ragged batch), which is eval-only '
                               '(no gradient exists for it)')
        if self._fwd_bt is None:
            raise RuntimeError('speechsplit_amd: input gradients need a preceding g3_forward / g6_forward on this engine')
        B, T = self._fwd_bt
        hp = self.hp
        shape = {'x_f0': (B, T, hp.dim_freq + hp.dim_f0), 'x_org': (B, T, hp.dim_freq), 'c_trg': (B, hp.dim_spk_emb),
                 'f0_trg': (B, T, hp.dim_f0)}
        return tuple(self._new('d' + n, shape[n]) if n in inputs else None for n in names)

    def g3_backward(self, d_out, inputs=()):
        """loss.backward() for the last g3_forward: parameter gradients into the arena.  inputs: names among G3_INPUTS whose gradients
        are wanted as well (ss_g3_backward_inputs); they come back as fresh tensors (dx_f0, dx_org, dc_trg), None where not asked for.
        Without inputs the call is ss_g3_backward and returns None."""
        d_out = self._f(d_out)
        if not inputs:
            _capi.check(self.lib.ss_g3_backward(self.h, _ptr(d_out), _stream()))
            return None
        dx_f0, dx_org, dc_trg = self._input_grad_buffers(self.G3_INPUTS, inputs)
        _capi.check(self.lib.ss_g3_backward_inputs(self.h, _ptr(d_out), _ptr(dx_f0), _ptr(dx_org), _ptr(dc_trg), _stream()))
        return dx_f0, dx_org, dc_trg

    def g3_rhythm(self, x_org, lengths=None):
        """lengths: a ragged batch (ss_g3_rhythm_ragged); the code rows >= lengths[b] / freq_2 of row b are zeros."""
        B, T, _ = x_org.shape
        ln = self._lengths(lengths, B, T) if lengths is not None else None
        self._fwd_bt = None
        self._reserve_eval(B, T, False)
        x_org = self._f(x_org)
        codes = self._new('codes', (B, T // self.hp.freq_2, 2 * self.hp.dim_neck_2))
        if ln is not None:
            _capi.check(self.lib.ss_g3_rhythm_ragged(self.h, _ptr(x_org), _ptr(ln), B, T, _ptr(codes), _stream()))
            return codes
        _capi.check(self.lib.ss_g3_rhythm(self.h, _ptr(x_org), B, T, _ptr(codes), _stream()))
        return codes

    # ------------------------------------------------------------------ codes (eval mode only)
    def code_shapes(self, B, T):
        """{name: shape} of the dense codes of a (B, T) batch: 'x' (content, Generator_3 only), 'r' (rhythm), 'f0' (pitch)."""
        hp = self.hp
        s = {'r': (B, T // hp.freq_2, 2 * hp.dim_neck_2), 'f0': (B, T // hp.freq_3, 2 * hp.dim_neck_3)}
        if self.kind == 'G3':
            s['x'] = (B, T // hp.freq, 2 * hp.dim_neck)
        return s

    def _codes_call(self, B, T, lengths):
        """What the four code calls share: lengths -> device i32[B], no forward left to differentiate, workspace reserved as g3_rhythm does."""
        ln = self._lengths(lengths, B, T) if lengths is not None else None
        self._fwd_bt = None
        self._reserve_eval(B, T, False)
        return ln

    def _code_arg(self, name, t, shape):
        t = self._f(t)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f'speechsplit_amd: {name} must have shape {tuple(shape)}, got {tuple(t.shape)}')
        return t

    def _want(self, want, names):
        want = tuple(names) if want is None else tuple(want)
        if not want or set(want) - set(names):
            raise ValueError(f'speechsplit_amd: want must name at least one of {tuple(names)}, got {want}')
        return want

    def g3_encode(self, x_f0, x_org, lengths=None, want=None):
        """The encoders of an eval-mode forward alone (ss_g3_encode) -> (codes_x, codes_r, codes_f0), dense [B, T / factor, 2 * dim_neck*].
        want: names among ('x', 'r', 'f0') to compute the codes for (default all); the others come back as None.
        lengths: a ragged batch; the code rows >= lengths[b] / factor of row b are zeros."""
        B, T, _ = x_org.shape
        want = self._want(want, ('x', 'r', 'f0'))
        hp = self.hp
        x_f0 = self._code_arg('x_f0', x_f0, (B, T, hp.dim_freq + hp.dim_f0))
        x_org = self._code_arg('x_org', x_org, (B, T, hp.dim_freq))
        ln = self._codes_call(B, T, lengths)
        shp = self.code_shapes(B, T)
        cx, cr, cf = (self._new('codes_' + n, shp[n]) if n in want else None for n in ('x', 'r', 'f0'))
        _capi.check(self.lib.ss_g3_encode(self.h, _ptr(x_f0), _ptr(x_org), _ptr(ln), B, T, _ptr(cx), _ptr(cr), _ptr(cf), _stream()))
        return cx, cr, cf

    def g3_decode(self, codes_x, codes_r, codes_f0, c_trg, lengths=None):
        """The decoder and head of an eval-mode forward on codes the caller supplies (ss_g3_decode) -> mel [B, T, dim_freq], T = freq_2 *
        codes_r.shape[1].  c_trg: [B, dim_spk_emb], or one row for every utterance.  lengths: a ragged batch; code rows at or beyond
        lengths[b] / factor are never read, output frames >= lengths[b] are zeros."""
        hp = self.hp
        if codes_r.dim() != 3:
            raise ValueError(f'speechsplit_amd: codes_r must be [B, T / freq_2, 2 * dim_neck_2], got {tuple(codes_r.shape)}')
        B, T = codes_r.shape[0], codes_r.shape[1] * hp.freq_2
        if T % hp.freq or T % hp.freq_3:
            raise ValueError(f'speechsplit_amd: codes_r implies T = {T}, which is not a multiple of the code factors {(hp.freq, hp.freq_2, hp.freq_3)}')
        shp = self.code_shapes(B, T)
        cx, cr, cf = (self._code_arg('codes_' + n, t, shp[n]) for n, t in (('x', codes_x), ('r', codes_r), ('f0', codes_f0)))
        c_trg = self._f(c_trg)
        if c_trg.dim() != 2 or c_trg.shape[1] != hp.dim_spk_emb or c_trg.shape[0] not in (1, B):
            raise ValueError(f'speechsplit_amd: c_trg must be [{B} or 1, {hp.dim_spk_emb}], got {tuple(c_trg.shape)}')
        if c_trg.shape[0] != B:
            c_trg = c_trg.expand(B, -1).contiguous()
        ln = self._codes_call(B, T, lengths)
        out = self._new('out', (B, T, hp.dim_freq))
        _capi.check(self.lib.ss_g3_decode(self.h, _ptr(cx), _ptr(cr), _ptr(cf), _ptr(c_trg), _ptr(ln), B, T, _ptr(out), _stream()))
        return out

    def g6_encode(self, x_org, f0_trg, lengths=None, want=None):
        """Generator_6's encoders alone (ss_g6_encode) -> (codes_r, codes_f0); want, lengths as g3_encode with the names ('r', 'f0')."""
        B, T, _ = x_org.shape
        want = self._want(want, ('r', 'f0'))
        hp = self.hp
        x_org = self._code_arg('x_org', x_org, (B, T, hp.dim_freq))
        f0_trg = self._code_arg('f0_trg', f0_trg, (B, T, hp.dim_f0))
        ln = self._codes_call(B, T, lengths)
        shp = self.code_shapes(B, T)
        cr, cf = (self._new('codes_' + n, shp[n]) if n in want else None for n in ('r', 'f0'))
        _capi.check(self.lib.ss_g6_encode(self.h, _ptr(x_org), _ptr(f0_trg), _ptr(ln), B, T, _ptr(cr), _ptr(cf), _stream()))
        return cr, cf

    def g6_decode(self, codes_r, codes_f0, lengths=None):
        """Generator_6's decoder and head on the caller's codes (ss_g6_decode) -> logits [B, T, dim_f0]; lengths as g3_decode."""
        hp = self.hp
        if codes_r.dim() != 3:
            raise ValueError(f'speechsplit_amd: codes_r must be [B, T / freq_2, 2 * dim_neck_2], got {tuple(codes_r.shape)}')
        B, T = codes_r.shape[0], codes_r.shape[1] * hp.freq_2
        if T % hp.freq or T % hp.freq_3:
            raise ValueError(f'speechsplit_amd: codes_r implies T = {T}, which is not a multiple of the code factors {(hp.freq, hp.freq_2, hp.freq_3)}')
        shp = self.code_shapes(B, T)
        cr, cf = (self._code_arg('codes_' + n, t, shp[n]) for n, t in (('r', codes_r), ('f0', codes_f0)))
        ln = self._codes_call(B, T, lengths)
        out = self._new('out', (B, T, hp.dim_f0))
        _capi.check(self.lib.ss_g6_decode(self.h, _ptr(cr), _ptr(cf), _ptr(ln), B, T, _ptr(out), _stream()))
        return out

    # ------------------------------------------------------------------ differentiable decode (decoder + head + speaker rows on given codes)
    def _decode_args(self, codes, c_trg=None):
        """Shape checks of g3_decode / g6_decode for the calls that differentiate: codes in the engine's order, dense, no lengths."""
        hp = self.hp
        names = ('x', 'r', 'f0') if self.kind == 'G3' else ('r', 'f0')
        codes_r = codes[names.index('r')]
        if codes_r.dim() != 3:
            raise ValueError(f'speechsplit_amd: codes_r must be [B, T / freq_2, 2 * dim_neck_2], got {tuple(codes_r.shape)}')
        B, T = codes_r.shape[0], codes_r.shape[1] * hp.freq_2
        if T % hp.freq or T % hp.freq_3:
            raise ValueError(f'speechsplit_amd: codes_r implies T = {T}, which is not a multiple of the code factors {(hp.freq, hp.freq_2, hp.freq_3)}')
        shp = self.code_shapes(B, T)
        codes = tuple(self._code_arg('codes_' + n, t, shp[n]) for n, t in zip(names, codes))
        if c_trg is not None:
            c_trg = self._f(c_trg)
            if c_trg.dim() != 2 or c_trg.shape[1] != hp.dim_spk_emb or c_trg.shape[0] not in (1, B):
                raise ValueError(f'speechsplit_amd: c_trg must be [{B} or 1, {hp.dim_spk_emb}], got {tuple(c_trg.shape)}')
            if c_trg.shape[0] != B:
                c_trg = c_trg.expand(B, -1).contiguous()
        self._fwd_bt = None
        return B, T, codes, c_trg

    def g3_decode_train(self, codes_x, codes_r, codes_f0, c_trg):
        """g3_decode on a dense batch, recorded so that g3_decode_backward can follow (ss_g3_decode_train): T <= max_frames, no lengths."""
        B, T, (cx, cr, cf), c_trg = self._decode_args((codes_x, codes_r, codes_f0), c_trg)
        out = self._new('out', (B, T, self.hp.dim_freq))
        _capi.check(self.lib.ss_g3_decode_train(self.h, _ptr(cx), _ptr(cr), _ptr(cf), _ptr(c_trg), B, T, _ptr(out), _stream()))
        self._dec_bt = (B, T)
        return out

    def _decode_grad_buffers(self, names, want):
        want = tuple(want)
        if set(want) - set(names):
            raise ValueError(f'speechsplit_amd: want must name some of {tuple(names)}, got {want}')
        B, T = getattr(self, '_dec_bt', None) or (1, self.hp.freq_2)      # (no decode ran: the call refuses; the buffers are never written)
        shp = dict(self.code_shapes(B, T), c_trg=(B, self.hp.dim_spk_emb))
        return tuple(self._new('d_' + n, shp[n]) if n in want else None for n in names)

    def g3_decode_backward(self, d_out, want=(), accumulate=False):
        """Backward of the last g3_decode_train (ss_g3_decode_backward): decoder + head gradients into the arena's [grad_split, arena)
        (the rest exact zeros unless accumulate).  want: names among ('x', 'r', 'f0', 'c_trg') -> (d_codes_x, d_codes_r, d_codes_f0,
        dc_trg) as fresh tensors, None where not asked for; dc_trg is per row [B, dim_spk_emb]."""
        dx, dr, df, dc = self._decode_grad_buffers(('x', 'r', 'f0', 'c_trg'), want)
        d_out = self._f(d_out)
        _capi.check(self.lib.ss_g3_decode_backward(self.h, _ptr(d_out), _ptr(dx), _ptr(dr), _ptr(df), _ptr(dc), step_flags(accumulate=accumulate), _stream()))
        return dx, dr, df, dc

    def g3_decode_train_step(self, codes_x, codes_r, codes_f0, c_trg, target_mel, grad_scale=1.0, no_adam=False, accumulate=False,
                             want_dc_trg=False):
        """Decode, MSE (mean) against target_mel, backward, Adam over the decoder + head range, in one call (ss_g3_decode_train_step).
        Returns the device loss, or (loss, dc_trg [B, dim_spk_emb]) with want_dc_trg.  no_adam: stop behind the backward."""
        self._no_training_on_ema('g3_decode_train_step')
        B, T, (cx, cr, cf), c_trg = self._decode_args((codes_x, codes_r, codes_f0), c_trg)
        tgt = self._code_arg('target_mel', target_mel, (B, T, self.hp.dim_freq))
        dc = self._new('d_c_trg', (B, self.hp.dim_spk_emb)) if want_dc_trg else None
        self._dec_bt = (B, T)
        flags = step_flags(no_adam=no_adam, accumulate=accumulate)
        _capi.check(self.lib.ss_g3_decode_train_step(self.h, _ptr(cx), _ptr(cr), _ptr(cf), _ptr(c_trg), _ptr(tgt), B, T, float(grad_scale), flags,
                                                     _ptr(self.loss), _ptr(dc), _stream()))
        return (self.loss, dc) if want_dc_trg else self.loss

    def g6_decode_train(self, codes_r, codes_f0):
        """g6_decode on a dense batch, recorded for g6_decode_backward (ss_g6_decode_train)."""
        B, T, (cr, cf), _ = self._decode_args((codes_r, codes_f0))
        out = self._new('out', (B, T, self.hp.dim_f0))
        _capi.check(self.lib.ss_g6_decode_train(self.h, _ptr(cr), _ptr(cf), B, T, _ptr(out), _stream()))
        self._dec_bt = (B, T)
        return out

    def g6_decode_backward(self, d_out, want=(), accumulate=False):
        """Backward of the last g6_decode_train (ss_g6_decode_backward); want: names among ('r', 'f0') -> (d_codes_r, d_codes_f0)."""
        dr, df = self._decode_grad_buffers(('r', 'f0'), want)
        d_out = self._f(d_out)
        _capi.check(self.lib.ss_g6_decode_backward(self.h, _ptr(d_out), _ptr(dr), _ptr(df), step_flags(accumulate=accumulate), _stream()))
        return dr, df

    def adam_step_decoder(self, grad_scale=1.0):
        """Adam on the decoder + head range [grad_split, arena) alone (ss_adam_step_decoder); the step counter advances by one."""
        self._no_training_on_ema('adam_step_decoder')
        _capi.check(self.lib.ss_adam_step_decoder(self.h, float(grad_scale), _stream()))

    def g3_train_step(self, mel, f0, emb, len_org, draws, grad_scale=1.0, no_adam=False, split_backward=False, bucket=False,
                      accumulate=False, split_no_join=False):
        """solver.py:160-172 fused.  split_backward: return after the decoder + head gradients (arena offsets >=
        self.grad_split) are complete; train_finish() then runs the encoder backward (data-parallel overlap); split_no_join: without
        joining the engine stream that carries the decoder's weight gradients (SS_STEP_SPLIT_NO_JOIN).
        bucket: the batch's frame count is its length bucket and the step runs with max_len_pad = T (SS_STEP_BUCKET).
        accumulate: the backward ADDS to the gradient arena (SS_STEP_ACCUMULATE).  A cycle of k micro-batches: no_adam=True, then
        no_adam=True + accumulate=True k - 2 times, then accumulate=True with grad_scale = 1 / k."""
        self._no_training_on_ema('g3_train_step')
        B, T, _ = mel.shape
        self._fwd_bt = None
        mel, f0, emb, len_org = self._f(mel), self._f(f0), self._f(emb), self._i(len_org)
        sc, ls = self._draws(draws)
        assert sc.shape[0] == 4 and ls.shape[0] == 4
        flags = step_flags(no_adam, split_backward, split_no_join, accumulate, bucket)
        _capi.check(self.lib.ss_g3_train_step(self.h, _ptr(mel), _ptr(f0), _ptr(emb), _ptr(len_org), _ptr(sc), _ptr(ls),
                                              B, T, float(grad_scale), flags, _ptr(self.loss), _stream()))
        return self.loss

    def train_finish(self, grad_scale=1.0, no_adam=True):
        self._no_training_on_ema('train_finish')
        _capi.check(self.lib.ss_train_finish(self.h, float(grad_scale), step_flags(no_adam=no_adam), _stream()))

    @property
    def grad_split(self):
        return int(self.lib.ss_grad_split(self.h))

    def dp_train_step(self, mel, f0, emb, len_org, draws, world, group=None, schedule='overlap', bucket=False, accumulate=False):
        """One data-parallel Generator_3 step on this rank's shard: backward, sum of the gradient arena over the ranks in the
        two buckets of dist.bucket_plan (decoder + head + status slot first, then the encoder), the same Adam update on every
        rank with the 1/world mean folded in.  Collectives: torch.distributed (backend 'nccl' = RCCL); the native path without
        PyTorch in the data path is dp_train_step_native.

        schedule='overlap' (default): the backward is enqueued exactly as in the one-GPU step (SS_STEP_SPLIT_NO_JOIN: the
            decoder's weight-gradient GEMMs stay on an engine stream beside the encoder backward); the first bucket's
            all-reduce is issued from a stream ordered behind the decoder chain and those GEMMs, BEFORE the encoder backward is
            enqueued, so it can run beside it.  (ProcessGroupNCCL launches the collective on its own internal stream, which
            first waits for the stream the call was issued from.)  Unmeasured at world > 1 on hardware: the one-GPU boxes this
            was developed on elide the collective.
        schedule='after': the one-GPU step unchanged, then the buckets; nothing hidden.
        schedule='join': SS_STEP_SPLIT_BACKWARD joins the engine streams, first bucket reduced right away (+0.6 ms at world 1:
            the decoder's weight-gradient GEMMs then run alone instead of beside the encoder backward).

        accumulate: this call is the LAST micro-batch of an accumulation cycle whose earlier ones went through
        g3_train_step(no_adam=True[, accumulate=True]) without any collective: its backward adds to the arena, the buckets reduce the
        local sums and Adam steps with 1 / (world * grad_accum_count)."""
        self._no_training_on_ema('dp_train_step')
        from . import dist as D
        self._fwd_bt = None
        k = self.grad_split
        plan = D.bucket_plan(self.grads.numel(), k)
        side = self.lib.ss_side_stream(self.h) if schedule == 'overlap' else None
        if schedule == 'overlap' and not side:
            schedule = 'after'                         # engine without branch streams
        if schedule == 'after':
            self.g3_train_step(mel, f0, emb, len_org, draws, no_adam=True, bucket=bucket, accumulate=accumulate)
            handles = [D.reduce_bucket(self.grads, lo, hi, group) for lo, hi in plan]
        elif schedule == 'join':
            self.g3_train_step(mel, f0, emb, len_org, draws, no_adam=True, split_backward=True, bucket=bucket, accumulate=accumulate)
            handles = [D.reduce_bucket(self.grads, *plan[0], group)]
            self.train_finish(no_adam=True)
            handles.append(D.reduce_bucket(self.grads, *plan[1], group))
        elif schedule == 'overlap':
            sc, ls = self._draws(draws)
            B, T, _ = mel.shape
            mel, f0, emb, len_org = self._f(mel), self._f(f0), self._f(emb), self._i(len_org)
            flags = step_flags(no_adam=True, split_backward=True, split_no_join=True, accumulate=accumulate, bucket=bucket)
            _capi.check(self.lib.ss_g3_train_step(self.h, _ptr(mel), _ptr(f0), _ptr(emb), _ptr(len_org), _ptr(sc), _ptr(ls),
                                                  B, T, 1.0, flags, _ptr(self.loss), _stream()))
            if getattr(self, '_side_stream', None) is None:
                self._side_stream = torch.cuda.ExternalStream(side, device=self.device)
            cs = self._side_stream
            # order the issuing stream behind the decoder chain and its weight-gradient GEMMs; this must precede the encoder
            # backward (a cross-stream wait on ROCm covers what the other stream holds when it is issued)
            _capi.check(self.lib.ss_wait_decoder_grads(self.h, C.c_void_p(cs.cuda_stream)))
            with torch.cuda.stream(cs):
                handles = [D.reduce_bucket(self.grads, *plan[0], group)]
            self.train_finish(no_adam=True)
            handles.append(D.reduce_bucket(self.grads, *plan[1], group))
        else:
            raise ValueError(f'unknown data-parallel schedule {schedule!r}')
        for h in handles:
            if h is not None:
                h.wait()                               # the current stream waits for the collectives
        self.adam_step(1.0 / (world * max(self.grad_accum_count, 1)))
        return self.loss

    def dp_g6_train_step(self, mel, f0_onehot, target_idx, draws, world, group=None, bucket=False, accumulate=False):
        """Data-parallel Generator_6 step (BASELINE config 4): the arena is 14 MB, one pass of the bucket plan behind the backward.
        accumulate: the last micro-batch of an accumulation cycle, as in dp_train_step."""
        self._no_training_on_ema('dp_g6_train_step')
        from . import dist as D
        self.g6_train_step(mel, f0_onehot, target_idx, draws, no_adam=True, bucket=bucket, accumulate=accumulate)
        D.reduce_arena(self.grads, self.grad_split, group)
        self.adam_step(1.0 / (world * max(self.grad_accum_count, 1)))
        return self.loss

    # ---- native RCCL (no PyTorch in the data path): ss_comm_* / ss_g3_dp_train_step of the C ABI
    def comm_init(self, rank=0, world=1, group=None):
        """Create this engine's RCCL communicator.  Rank 0 draws the 128-byte id; with world > 1 it is handed round through the
        already initialised torch.distributed group (any backend: it is 128 bytes of bootstrap, not data)."""
        buf = C.create_string_buffer(128)
        if rank == 0:
            _capi.check(self.lib.ss_comm_unique_id(buf))
        if world > 1:
            import torch.distributed as dist
            box = [bytes(buf.raw)]
            dist.broadcast_object_list(box, src=0, group=group)
            buf = C.create_string_buffer(box[0], 128)
        _capi.check(self.lib.ss_comm_init(self.h, buf, int(rank), int(world)))
        self.comm_world = int(world)

    def scratch_fallbacks(self):
        """Launches that found the step's scratch exhausted and took their slower path (ss_scratch_fallbacks); 0 in a healthy run."""
        return int(self.lib.ss_scratch_fallbacks(self.h))

    def dp_profile(self, on=True):
        """hipEvent brackets round every collective of the native data-parallel steps (ss_dp_profile)."""
        _capi.check(self.lib.ss_dp_profile(self.h, 1 if on else 0))

    def dp_profile_read(self):
        """[(arena offset or -1 for the grouped rest, elements, start_us, end_us)] of the last data-parallel step's collectives, times
        relative to the end of the backward on the main stream (negative: hidden beside it).  Synchronises."""
        n = self.lib.ss_dp_profile_read(self.h, None, 0)
        if n <= 0:
            return []
        buf = (C.c_double * (4 * n))()
        n = self.lib.ss_dp_profile_read(self.h, buf, n)
        if n < 0:
            _capi.check(n)
        return [(int(buf[4 * i]), int(buf[4 * i + 1]), float(buf[4 * i + 2]), float(buf[4 * i + 3])) for i in range(n)]

    def allreduce_grads(self, lo=0, hi=None):
        hi = self.grads.numel() if hi is None else hi
        _capi.check(self.lib.ss_allreduce_grads(self.h, int(lo), int(hi - lo), _stream()))

    def dp_train_step_native(self, mel, f0, emb, len_org, draws, bucket=False, accumulate=False):
        """ss_g3_dp_train_step: the overlapped two-bucket schedule with the collectives launched by the engine itself, the
        decoder bucket ON the engine stream that carries the decoder's weight-gradient GEMMs.  accumulate: the last micro-batch of an
        accumulation cycle (SS_STEP_ACCUMULATE): the buckets reduce the local sums, Adam steps with 1 / (world * grad_accum_count)."""
        self._no_training_on_ema('dp_train_step_native')
        self._fwd_bt = None
        B, T, _ = mel.shape
        mel, f0, emb, len_org = self._f(mel), self._f(f0), self._f(emb), self._i(len_org)
        sc, ls = self._draws(draws)
        _capi.check(self.lib.ss_g3_dp_train_step(self.h, _ptr(mel), _ptr(f0), _ptr(emb), _ptr(len_org), _ptr(sc), _ptr(ls), B, T,
                                                 step_flags(accumulate=accumulate, bucket=bucket), _ptr(self.loss), _stream()))
        return self.loss

    # ------------------------------------------------------------------ Generator_6
    def g6_forward(self, x_org, f0_trg, draws=None, training=False, lengths=None):
        """lengths (eval mode only): a ragged batch, as g3_forward (ss_g6_forward_ragged)."""
        B, T, _ = x_org.shape
        ln = self._lengths(lengths, B, T, training) if lengths is not None else None
        x_org, f0_trg = self._f(x_org), self._f(f0_trg)
        sc, ls = self._draws(draws)
        out = self._new('out', (B, T, self.hp.dim_f0))
        self._fwd_bt = None
        self._reserve_eval(B, T, training)
        if ln is not None:
            _capi.check(self.lib.ss_g6_forward_ragged(self.h, _ptr(x_org), _ptr(f0_trg), _ptr(ln), B, T, 0, _ptr(out), _stream()))
            self._fwd_bt = RAGGED
            return out
        _capi.check(self.lib.ss_g6_forward(self.h, _ptr(x_org), _ptr(f0_trg), _ptr(sc), _ptr(ls), B, T, int(training),
                                           _ptr(out), _stream()))
        self._fwd_bt = (B, T)
        return out

    def g6_backward(self, d_out, inputs=()):
        """As g3_backward for Generator_6: inputs among G6_INPUTS, returns (dx_org, df0_trg) when any is asked for."""
        d_out = self._f(d_out)
        if not inputs:
            _capi.check(self.lib.ss_g6_backward(self.h, _ptr(d_out), _stream()))
            return None
        dx_org, df0_trg = self._input_grad_buffers(self.G6_INPUTS, inputs)
        _capi.check(self.lib.ss_g6_backward_inputs(self.h, _ptr(d_out), _ptr(dx_org), _ptr(df0_trg), _stream()))
        return dx_org, df0_trg

    def g6_train_step(self, mel, f0_onehot, target_idx, draws, grad_scale=1.0, no_adam=False, bucket=False, accumulate=False):
        """accumulate: the backward adds to the gradient arena (SS_STEP_ACCUMULATE), as in g3_train_step."""
        self._no_training_on_ema('g6_train_step')
        self._fwd_bt = None
        B, T, _ = mel.shape
        mel, f0_onehot, target_idx = self._f(mel), self._f(f0_onehot), self._i(target_idx)
        sc, ls = self._draws(draws)
        _capi.check(self.lib.ss_g6_train_step(self.h, _ptr(mel), _ptr(f0_onehot), _ptr(target_idx), _ptr(sc), _ptr(ls), B, T,
                                              float(grad_scale), step_flags(no_adam=no_adam, accumulate=accumulate, bucket=bucket), _ptr(self.loss),
                                              _stream()))
        return self.loss

    def g6_dp_train_step_native(self, mel, f0_onehot, target_idx, draws, bucket=False, accumulate=False):
        """ss_g6_dp_train_step: Generator_6's data-parallel step with the engine's own RCCL communicator (per-layer buckets on the
        engine's communication stream), as dp_train_step_native for Generator_3."""
        self._no_training_on_ema('g6_dp_train_step_native')
        self._fwd_bt = None
        B, T, _ = mel.shape
        mel, f0_onehot, target_idx = self._f(mel), self._f(f0_onehot), self._i(target_idx)
        sc, ls = self._draws(draws)
        _capi.check(self.lib.ss_g6_dp_train_step(self.h, _ptr(mel), _ptr(f0_onehot), _ptr(target_idx), _ptr(sc), _ptr(ls), B, T,
                                                 step_flags(accumulate=accumulate, bucket=bucket), _ptr(self.loss), _stream()))
        return self.loss

    # ------------------------------------------------------------------ optimiser / misc
    def adam_step(self, grad_scale=1.0):
        self._no_training_on_ema('adam_step')
        _capi.check(self.lib.ss_adam_step(self.h, float(grad_scale), _stream()))

    def set_grad_clip(self, max_norm):
        """torch.nn.utils.clip_grad_norm_(parameters, max_norm) inside every optimiser step of this engine, on the device (ss_set_grad_clip):
        None / 0 off (default), > 0 clip to that global norm, inf measure only.  With it on, a step whose gradient norm is not finite is
        skipped (parameters, moments and step counter untouched) and counted; the counters of grad_clip_stats() start again."""
        _capi.check(self.lib.ss_set_grad_clip(self.h, float(max_norm or 0.0), _stream()))

    def grad_norm(self, grad_scale=1.0):
        """grad_scale * 2-norm of the parameter elements of the gradient arena as it is now: a one-element device tensor (ss_grad_norm)."""
        out = self._new('grad_norm', (1,))
        _capi.check(self.lib.ss_grad_norm(self.h, float(grad_scale), _ptr(out), _stream()))
        return out

    def grad_clip_stats(self):
        """Device tensor [4], no synchronisation (ss_grad_clip_stats): norm of the last optimiser step before clipping, coefficient applied
        (0: skipped), optimiser steps clipped, optimiser steps skipped as non-finite -- the counts since set_grad_clip."""
        out = self._new('grad_clip_stats', (4,))
        _capi.check(self.lib.ss_grad_clip_stats(self.h, _ptr(out), _stream()))
        return out

    # ------------------------------------------------------------------ weight decay / parameter EMA
    WD_WHICH = {'all': 0, 'weights': 1}
    ema = None                             # the average's arena while set_ema is on (a flat tensor like params)
    _ema_swapped = False

    def set_weight_decay(self, wd, which='all'):
        """torch.optim.AdamW's decoupled weight decay inside every optimiser step (ss_set_weight_decay): None / 0 off (default).  which:
        'all' every parameter (AdamW(G.parameters(), weight_decay=wd)), 'weights' tensors with ndim >= 2 only (biases and the GroupNorm
        affine are left alone)."""
        if which not in self.WD_WHICH:
            raise ValueError(f"set_weight_decay: which must be 'all' or 'weights', not {which!r}")
        _capi.check(self.lib.ss_set_weight_decay(self.h, float(wd or 0.0), self.WD_WHICH[which], _stream()))

    def set_ema(self, decay, warmup=False, state=None):
        """An exponential moving average of the parameters, updated inside every applied optimiser step (ss_set_ema): ema += (1 - d) * (p - ema),
        d = decay, or with warmup min(decay, (1 + n) / (10 + n)).  decay None switches it off.  The arena comes from the engine's allocator
        ('ema') and is self.ema / ema_views().  state = (tensor, updates): resume from a flat arena-sized average and its update count;
        otherwise the average starts as a copy of the parameters with zero updates."""
        if self._ema_swapped:
            raise RuntimeError('set_ema inside ema_weights(): the parameters and their average are exchanged')
        if decay is None:
            _capi.check(self.lib.ss_set_ema(self.h, None, 0.0, 0, 0, _stream()))
            self.ema = None
            return
        if self.ema is None:
            with torch.cuda.device(self.device):
                self.ema = self._new('ema', (self.params.numel(),), zero=True)
        updates = -1
        if state is not None:
            t, updates = state
            t = torch.as_tensor(t)
            assert t.numel() == self.ema.numel() and int(updates) >= 0, 'set_ema: state = (arena-sized tensor, updates >= 0)'
            self.ema.copy_(t.reshape(-1).to(device=self.device, dtype=torch.float32))
        _capi.check(self.lib.ss_set_ema(self.h, _ptr(self.ema), float(decay), int(bool(warmup)), int(updates), _stream()))

    def ema_views(self):
        if self.ema is None:
            raise RuntimeError('ema_views: no EMA (call set_ema first)')
        return self.views(self.ema)

    def ema_stats(self):
        """Device tensor [4], no synchronisation (ss_ema_stats): EMA updates applied, d of the last update, weight-decay factor of the last
        applied step, 0."""
        out = self._new('ema_stats', (4,))
        _capi.check(self.lib.ss_ema_stats(self.h, _ptr(out), _stream()))
        return out

    # ------------------------------------------------------------------ learning-rate schedule
    LR_KINDS = {None: 0, 'off': 0, 'constant': 1, 'cosine': 2, 'linear': 3, 'exponential': 4, 'step': 5}

    def set_lr_schedule(self, kind=None, warmup=0, warmup_start=0.1, total=None, gamma=None, period=None, min_lr=0.0):
        """Warm-up and decay of the learning rate inside every applied optimiser step, keyed on the device's step counter
        (ss_set_lr_schedule; the definition is in include/speechsplit_amd.h).  kind: None / 'off' (default), 'constant', 'cosine', 'linear',
        'exponential' or 'step'.  warmup steps rise linearly from warmup_start * lr to lr; then cosine / linear reach min_lr after total
        steps and stay there, exponential multiplies by gamma every step and step by gamma every period steps, both floored at min_lr.
        The base rate stays the lr of set_adam, whose step positions the schedule."""
        if kind not in self.LR_KINDS:
            raise ValueError(f"set_lr_schedule: kind must be None, 'off', 'constant', 'cosine', 'linear', 'exponential' or 'step', not {kind!r}")
        k = self.LR_KINDS[kind]
        # an option its kind reads has no default: leaving it out is the engine's refusal, by name
        _capi.check(self.lib.ss_set_lr_schedule(self.h, k, int(warmup), float(warmup_start), int(total) if total is not None else 0,
                                                float(gamma) if gamma is not None else 0.0, int(period) if period is not None else 0,
                                                float(min_lr), _stream()))

    def lr_stats(self):
        """Device tensor [4], no synchronisation (ss_lr_stats): the learning rate of the last applied optimiser step, that rate over the
        base rate, the step t it belonged to, the schedule's kind (0 off)."""
        out = self._new('lr_stats', (4,))
        _capi.check(self.lib.ss_lr_stats(self.h, _ptr(out), _stream()))
        return out

    def ema_weights(self):
        """Context manager: the engine runs on the averaged weights inside (ss_ema_swap on entry and again on exit, which restores the
        parameters' bits).  Training and optimiser steps raise inside: they would train the average."""
        import contextlib

        @contextlib.contextmanager
        def swapped():
            if self.ema is None:
                raise RuntimeError('ema_weights: no EMA (call set_ema first)')
            if self._ema_swapped:
                raise RuntimeError('ema_weights: already inside ema_weights()')
            _capi.check(self.lib.ss_ema_swap(self.h, _stream()))
            self._ema_swapped = True
            try:
                yield self
            finally:
                self._ema_swapped = False
                _capi.check(self.lib.ss_ema_swap(self.h, _stream()))
        return swapped()

    def _no_training_on_ema(self, what):
        if self._ema_swapped:
            raise RuntimeError(f'{what} inside ema_weights(): the step would train the averaged weights')

    def check(self):
        """Synchronise and raise if a kernel reported an asynchronous failure."""
        _capi.check(self.lib.ss_check(self.h, _stream()))

    def status(self):
        """Engine status word without synchronising (ss_status): 0 ok, bit 0 aborted recurrence, 1 remote abort, 2 parameter range."""
        return int(self.lib.ss_status(self.h))

    def clear_abort(self):
        _capi.check(self.lib.ss_clear_abort(self.h, _stream()))

    def set_lockstep(self, on=True):
        """Data-parallel member whose gradients are exchanged outside the engine (torch.distributed): entry points never refuse on the
        status word, check() reports it at a point all ranks reach together (ss_set_lockstep; the native communicator sets it itself)."""
        _capi.check(self.lib.ss_set_lockstep(self.h, 1 if on else 0))

    def zero_grads(self):
        _capi.check(self.lib.ss_zero_grads(self.h, _stream()))

    @property
    def grad_accum_count(self):
        """Backward passes summed into the gradient arena since it was last cleared (ss_grad_accum_count; host-side)."""
        return int(self.lib.ss_grad_accum_count(self.h))

    def interp_forward(self, x, len_seq, scales, len_seg, want_plan=False, out=None):
        """out: optional pre-placed dense outputs (y, i0, lam, counts) instead of fresh ones (i0 / lam / counts may be None)."""
        B, T, Cc = x.shape
        P = self.hp.max_len_pad
        x, len_seq = self._f(x), self._i(torch.as_tensor(len_seq))
        sc, ls = self._f(torch.as_tensor(scales)), self._i(torch.as_tensor(len_seg))
        if out is not None:
            y, i0, lam, cnt = out
            assert all(t is None or t.is_contiguous() for t in out) and tuple(y.shape) == (B, P, Cc)
        else:
            y = torch.empty(B, P, Cc, device=self.device)
            i0 = torch.empty(B, P, dtype=torch.int32, device=self.device) if want_plan else None
            lam = torch.empty(B, P, device=self.device) if want_plan else None
            cnt = torch.empty(B, dtype=torch.int32, device=self.device) if want_plan else None
        _capi.check(self.lib.ss_interp_forward(self.h, _ptr(x), _ptr(len_seq), _ptr(sc), _ptr(ls), B, T, Cc, _ptr(y),
                                               _ptr(i0), _ptr(lam), _ptr(cnt), _stream()))
        return (y, i0, lam, cnt) if want_plan else y

    def interp_backward(self, dy, T, out=None):
        B, P, Cc = dy.shape
        dy = self._f(dy)
        dx = torch.empty(B, T, Cc, device=self.device) if out is None else out
        assert dx.is_contiguous() and tuple(dx.shape) == (B, T, Cc)
        _capi.check(self.lib.ss_interp_backward(self.h, _ptr(dy), B, T, Cc, _ptr(dx), _stream()))
        return dx

    def debug_names(self):
        buf = C.create_string_buffer(1 << 14)
        self.lib.ss_debug_names(self.h, buf, len(buf))
        return [s for s in buf.value.decode().split('\n') if s]

    def relu_masks(self, B, T):
        """Test hook (ss_debug_relu_mask): {conv block name: bool [B,T,Co]} -- the ReLU branch taken in the last forward."""
        out = {}
        for name in self.debug_names():
            if not name.endswith('.conv'):
                continue
            blk = name[:-5]
            p, rows, cols = C.c_void_p(), C.c_long(), C.c_long()
            _capi.check(self.lib.ss_debug_buffer(self.h, name.encode(), C.byref(p), C.byref(rows), C.byref(cols)))
            m = torch.empty(B, T, cols.value, device=self.device)
            _capi.check(self.lib.ss_debug_relu_mask(self.h, blk.encode(), _ptr(m), _stream()))
            out[blk] = m > 0
        return out

    def set_precision(self, precision):
        """'f32' (default, the 1e-4 parity mode) or 'bf16' (bf16-rounded GEMM operands, fp32 accumulate / state)."""
        code = {'f32': 0, 'fp32': 0, 'bf16': 1}[precision]
        _capi.check(self.lib.ss_set_precision(self.h, code))
        self.precision = 'bf16' if code else 'f32'

    PROF_CLASSES = ('dec_proj', 'dec_proj0', 'dec_dw', 'dec_dx', 'conv_fwd', 'conv_dw', 'conv_dx', 'rec_fwd', 'rec_bwd',
                    'enc_lstm', 'head')

    PROF_TIMELINE = ('enc_rec', 'gn', 'wgrad', 'adam', 'prep')      # timeline-only classes (SS_PROF_ENC_REC ..): non-GEMM launches, no flops

    def profile(self, classes, every=1):
        """ss_profile: bracket the launches of the named classes (True: all; False / empty: stop) with hipEvents; starting
        clears the record.  every = n: only every n-th training step is bracketed (ss_profile_sample)."""
        _capi.check(self.lib.ss_profile_sample(self.h, int(every)))
        names = self.PROF_CLASSES + self.PROF_TIMELINE
        if classes is True:
            mask = (1 << len(self.PROF_CLASSES)) - 1
        elif classes == 'timeline':                  # every class including the timeline-only ones
            mask = (1 << len(names)) - 1
        elif not classes:
            mask = 0
        else:
            mask = sum(1 << names.index(c) for c in classes)
        _capi.check(self.lib.ss_profile(self.h, mask))

    def profile_read(self):
        """{class: (launches, total_us, total_flops)} of the launches recorded since profile(True) (ss_profile_read)."""
        out = {}
        for k, name in enumerate(self.PROF_CLASSES):
            n, us, fl = C.c_int(), C.c_double(), C.c_double()
            _capi.check(self.lib.ss_profile_read(self.h, k, C.byref(n), C.byref(us), C.byref(fl)))
            if n.value:
                out[name] = (n.value, us.value, fl.value)
        return out

    def profile_timeline(self, cap=8192):
        """[(class name, start_us, end_us, stream)] of the recorded brackets in enqueue order, relative to the first one's start
        (ss_profile_timeline); stream: 0 main, 1 side, 2 / 3 the branch streams."""
        buf = (C.c_double * (3 * cap))()
        n = self.lib.ss_profile_timeline(self.h, buf, cap)
        if n < 0:
            _capi.check(n)
        names = self.PROF_CLASSES + self.PROF_TIMELINE
        return [(names[int(buf[3 * i]) % 100], buf[3 * i + 1], buf[3 * i + 2], int(buf[3 * i]) // 100) for i in range(n)]

    def debug_buffer(self, name, B, T, halo=False):
        """Real frames of an internal haloed slab as a [B, T, C] tensor (copy); halo=True: the whole slab [B, T + 4, C], halo rows included."""
        p, rows, cols = C.c_void_p(), C.c_long(), C.c_long()
        _capi.check(self.lib.ss_debug_buffer(self.h, name.encode(), C.byref(p), C.byref(rows), C.byref(cols)))
        off = p.value - self.ws.data_ptr()
        n = rows.value * cols.value
        flat = self.ws[off:off + 4 * n].view(torch.float32)
        slab = flat.view(B, T + 4, cols.value)
        return slab.clone() if halo else slab[:, 2:2 + T].clone()


def split_image(x, scale=16.0, out=None):
    """Test hook (ss_op_split_image): fp32 [rows, cols] (cols % 8 == 0) -> its operand image, a float32-typed tensor of the same shape whose
    bytes are, per 8 elements, 16 B of fp16 hi pieces and 16 B of fp16 lo pieces of scale * x (csrc/common.h, image format v2).  x may be a
    row-strided view (its row stride is passed on); out: a pre-placed image tensor of the same shape (row stride a multiple of 8)."""
    lib = _capi.lib()
    rows, cols = x.shape
    if x.stride(1) != 1:
        x = x.contiguous()
    img = torch.empty(rows, cols, device=x.device) if out is None else out
    assert tuple(img.shape) == (rows, cols) and img.stride(1) == 1
    _capi.check(lib.ss_op_split_image(_ptr(x), x.stride(0), rows, cols, float(scale), _ptr(img), img.stride(0), _stream()))
    return img


_ZEROS = {}


def gemm_img(a_img, b_img, ta=False, tb=False, bias=None, ksplit=1, cfg=-1, scale_a=16.0, scale_b=16.0, out=None, accumulate=False, a_seg=(0, 0),
             M=None, K=None, part=None, zeros=None):
    """Test hook (ss_op_gemm_img): C[M,N] = A(m,k) B(n,k) over operand images.  a_img [M,K] ([K,M] if ta), b_img [N,K] ([K,N] if tb).
    torch.bfloat16 operands select the single-piece form (plain bf16 matrices, no scales)."""
    lib = _capi.lib()
    bf16 = a_img.dtype == torch.bfloat16
    assert (b_img.dtype == torch.bfloat16) == bf16
    if M is None:
        M = a_img.shape[1] if ta else a_img.shape[0]
    if K is None:
        K = a_img.shape[0] if ta else a_img.shape[1]
    N = b_img.shape[1] if tb else b_img.shape[0]
    dev = a_img.device
    c = torch.zeros(M, N, device=dev) if out is None else out
    if ksplit > 1 and part is None:
        part = torch.empty(ksplit * M * N, device=dev)
    z = _ZEROS.setdefault(str(dev), torch.zeros(1024, device=dev)) if zeros is None else zeros     # zeros_dev: >= 1 KB of zero bytes
    _capi.check(lib.ss_op_gemm_img(_ptr(a_img), a_img.stride(0), _ptr(b_img), b_img.stride(0), _ptr(c), c.stride(0), _ptr(bias), M, N, K,
                                   (1 if ta else 0) | (2 if tb else 0) | (4 if accumulate else 0) | (8 if bf16 else 0), int(ksplit), int(cfg), float(scale_a),
                                   float(scale_b), int(a_seg[0]), int(a_seg[1]), _ptr(part), _ptr(z), _stream()))
    return c


def conv_block(x, w, bias, gamma, beta, dy=None, need_dx=True, scratch=None, out=None, lengths=None):
    """Test hook (ss_op_conv_block): relu(GroupNorm(conv5(x))) of one block through the engine's block routines.
    x [B,T,Ci] -> y [B,T,Co]; with dy also (dx, gw, gb, ggamma, gbeta).  The C ABI takes dense tensors: contiguous operands are passed where
    they lie (any base), others are copied.  scratch: pre-placed, at least ss_op_conv_block_scratch() floats; out: dict of pre-placed dense
    outputs by name (y, dx, gw, gb, ggamma, gbeta).  lengths: per-row frame counts of a ragged batch (ss_op_conv_block_ragged; forward only)."""
    lib = _capi.lib()
    B, T, Ci = x.shape
    Co = w.shape[0]
    dev = x.device
    f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    x, w, bias, gamma, beta = f(x), f(w), f(bias), f(gamma), f(beta)
    n = lib.ss_op_conv_block_scratch(B, T, Ci, Co)
    if scratch is None:
        scratch = torch.empty(n, device=dev)
    assert scratch.is_contiguous() and scratch.numel() >= n
    n = scratch.numel()
    out = out or {}

    def o(name, *shape):
        t = out.get(name)
        if t is None:
            return torch.empty(*shape, device=dev)
        assert tuple(t.shape) == shape and t.is_contiguous(), name
        return t
    y = o('y', B, T, Co)
    if lengths is not None:
        if dy is not None:
            raise ValueError('speechsplit_amd: a ragged conv block runs the forward only')
        ln = check_lengths(lengths, B, T, (1,), dev)
        _capi.check(lib.ss_op_conv_block_ragged(_ptr(x), _ptr(w), _ptr(bias), _ptr(gamma), _ptr(beta), _ptr(ln), _ptr(y), _ptr(scratch), n,
                                                B, T, Ci, Co, _stream()))
        return y
    if dy is None:
        _capi.check(lib.ss_op_conv_block(_ptr(x), _ptr(w), _ptr(bias), _ptr(gamma), _ptr(beta), None, _ptr(y), None, None, None,
                                         None, None, _ptr(scratch), n, B, T, Ci, Co, _stream()))
        return y
    dy = f(dy)
    dx = o('dx', B, T, Ci) if need_dx else None
    gw, gb, gg, gbe = o('gw', *w.shape), o('gb', Co), o('ggamma', Co), o('gbeta', Co)
    _capi.check(lib.ss_op_conv_block(_ptr(x), _ptr(w), _ptr(bias), _ptr(gamma), _ptr(beta), _ptr(dy), _ptr(y), _ptr(dx), _ptr(gw),
                                     _ptr(gb), _ptr(gg), _ptr(gbe), _ptr(scratch), n, B, T, Ci, Co, _stream()))
    return y, dx, gw, gb, gg, gbe


def check_gn_plan(T, P, i0=None, lam=None, nrows=None, start=None):
    """The plan contract of ss_op_gn_relu_fwd / _bwd (include/speechsplit_amd.h), asserted on the HOST before a launch -- the hooks cannot see
    the contents of a device-resident plan, and a plan outside the contract would make the kernels index outside their tiles.  Raises
    ValueError.  (Test hooks: the device-to-host copy this takes is of no concern.)"""
    if not 1 <= P <= 258:
        raise ValueError(f'speechsplit_amd: plan: P = {P} outside 1 .. 258')
    B = None
    for name, t, shape_tail, dt in (('i0', i0, (P,), torch.int32), ('lam', lam, (P,), torch.float32), ('nrows', nrows, (), torch.int32),
                                    ('start', start, (T + 1,), torch.int32)):
        if t is None:
            continue
        if t.dtype != dt or not t.is_contiguous() or tuple(t.shape[1:]) != shape_tail or (B is not None and t.shape[0] != B):
            raise ValueError(f'speechsplit_amd: plan: {name} must be a contiguous {dt} tensor [B{"".join(f", {s}" for s in shape_tail)}]')
        B = t.shape[0]
    if nrows is not None:
        n = nrows.cpu().numpy()
        if (n < 0).any() or (n > P).any():
            raise ValueError('speechsplit_amd: plan: nrows outside 0 .. P')
        if i0 is not None:
            h = i0.cpu().numpy()
            for b in range(B):
                live = h[b, :n[b]]
                if live.size and (live.min() < 0 or live.max() >= T or (np.diff(live) < 0).any()):
                    raise ValueError(f'speechsplit_amd: plan: i0[{b}] leaves 0 .. T - 1 or decreases within its live rows')
    if lam is not None and not bool(torch.isfinite(lam).all()):
        raise ValueError('speechsplit_amd: plan: lam is not finite')
    if start is not None:
        s = start.cpu().numpy()
        if (s < 0).any() or (s > P).any() or (np.diff(s, axis=1) < 0).any() or (s[:, 0] != 0).any():
            raise ValueError('speechsplit_amd: plan: start must rise from 0 and stay within 0 .. P')
        if nrows is not None and (s[:, T] != nrows.cpu().numpy()).any():
            raise ValueError('speechsplit_amd: plan: start[b][T] != nrows[b]')
    return B


def gn_plan_start(i0, nrows, T):
    """start [B, T+1] i32 as csrc/interp.hip defines it: start[b][i] = number of rows r < nrows[b] with i0[b][r] < i."""
    h, n = i0.cpu().numpy(), nrows.cpu().numpy()
    st = np.stack([np.searchsorted(h[b, :n[b]], np.arange(T + 1), side='left') for b in range(h.shape[0])]).astype(np.int32)
    return torch.from_numpy(st).to(i0.device)


def _gn_rows(t, B, rows, C, name):
    """A haloed slab view [B, rows + 4, C] with unit channel stride -> (pointer to slab row 0, ld, bs)."""
    if t.dim() != 3 or tuple(t.shape) != (B, rows + 4, C) or t.stride(2) != 1 or t.dtype != torch.float32:
        raise ValueError(f'speechsplit_amd: {name} must be a float32 slab view [B, {rows} + 4, C] with unit channel stride, got {tuple(t.shape)}')
    return _ptr(t), t.stride(1), (t.stride(0) if B > 1 else (rows + 4) * t.stride(1))


def gn_relu_scratch(B, T, C):
    """Bytes of scratch gn_relu_fwd needs (ss_op_gn_relu_scratch): 0 for T <= 256."""
    return int(_capi.lib().ss_op_gn_relu_scratch(B, T, C))


def gn_relu_fwd(x, y, gamma, beta, stats, lengths=None, plan=None, y_img=None, img_scale=None, scratch=None):
    """Test hook (ss_op_gn_relu_fwd): the GroupNorm + ReLU forward kernels on the CALLER's haloed slabs, nothing copied.  x [B, T+4, C] and y
    [B, T+4, C] (gather form: [B, P+4, C]) are slab VIEWS (any row / batch stride the header allows); gamma / beta [C]; stats [B, C/16, 2] is
    written.  lengths: device i32[B], the ragged form.  plan = (i0 [B,P] i32, lam [B,P] f32, nrows [B] i32): the gather form; the plan
    contract is asserted on the host first (check_gn_plan).  y_img: the image of y in y's geometry -- a float32 view like y (format v2, split
    with the device word img_scale, None: 16) or a bfloat16 view like y (plain bf16).  scratch: a tensor of at least gn_relu_scratch(B, T, C)
    bytes for T > 256."""
    B, TP, Cc = x.shape
    T = TP - 4
    xp, x_ld, x_bs = _gn_rows(x, B, T, Cc, 'x')
    i0 = lam = nrows = None
    P = 0
    if plan is not None:
        i0, lam, nrows = plan
        P = i0.shape[1]
        if check_gn_plan(T, P, i0=i0, lam=lam, nrows=nrows) != B:
            raise ValueError('speechsplit_amd: plan: batch size differs from x')
    yp, y_ld, y_bs = _gn_rows(y, B, P if plan is not None else T, Cc, 'y')
    bf16 = y_img is not None and y_img.dtype == torch.bfloat16
    if y_img is not None:
        if tuple(y_img.shape) != tuple(y.shape) or y_img.stride() != y.stride() or y_img.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("speechsplit_amd: y_img must have y's shape and strides (float32: format v2, bfloat16: plain)")
    if lengths is not None and (lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,) or not lengths.is_contiguous()):
        raise ValueError('speechsplit_amd: lengths must be a contiguous device i32[B]')
    assert gamma.is_contiguous() and beta.is_contiguous() and stats.is_contiguous() and tuple(stats.shape) == (B, Cc // 16, 2)
    _capi.check(_capi.lib().ss_op_gn_relu_fwd(xp, x_ld, x_bs, yp, y_ld, y_bs, _ptr(gamma), _ptr(beta), _ptr(stats), _ptr(lengths), _ptr(i0), _ptr(lam),
                                              _ptr(nrows), P, _ptr(y_img), _ptr(img_scale), 1 if bf16 else 0, _ptr(scratch),
                                              scratch.numel() * scratch.element_size() if scratch is not None else 0, B, T, Cc, _stream()))
    return y


def gn_relu_mask(x, gamma, beta, stats, out=None):
    """Test hook (ss_op_gn_relu_mask): mask [B, T, C] dense, 1.0 where the GroupNorm output is > 0 -- the branch the kernels take."""
    B, TP, Cc = x.shape
    T = TP - 4
    xp, x_ld, x_bs = _gn_rows(x, B, T, Cc, 'x')
    m = torch.empty(B, T, Cc, device=x.device) if out is None else out
    assert m.is_contiguous() and tuple(m.shape) == (B, T, Cc)
    _capi.check(_capi.lib().ss_op_gn_relu_mask(xp, x_ld, x_bs, _ptr(gamma), _ptr(beta), _ptr(stats), _ptr(m), B, T, Cc, _stream()))
    return m


def gn_relu_bwd(x, dy, gamma, beta, stats, g_gamma, g_beta, g_bias, amax=None, part=None, scatter=None, src=None, dy_img=None):
    """Test hook (ss_op_gn_relu_bwd): the GroupNorm + ReLU backward kernel on the caller's slabs.  x, dy [B, T+4, C] slab views; dy is
    replaced in place by the gradient of x; g_gamma / g_beta / g_bias [C] are accumulated into.  amax: one float32 word; part: [B, 3, C]
    (used under tune('deterministic', 1) only).  scatter = (lam [B,P] f32, start [B,T+1] i32) with src [B, P+4, C] (slab view): the fused
    adjoint of the gather -- the contract is asserted on the host first.  dy_img: a bfloat16 view with dy's shape and strides."""
    B, TP, Cc = x.shape
    T = TP - 4
    xp, x_ld, x_bs = _gn_rows(x, B, T, Cc, 'x')
    dp, d_ld, d_bs = _gn_rows(dy, B, T, Cc, 'dy')
    lam = start = None
    P, sp, s_ld, s_bs = 0, C.c_void_p(0), 0, 0
    if scatter is not None:
        lam, start = scatter
        P = lam.shape[1]
        if check_gn_plan(T, P, lam=lam, start=start) != B:
            raise ValueError('speechsplit_amd: plan: batch size differs from x')
        sp, s_ld, s_bs = _gn_rows(src, B, P, Cc, 'src')
    if dy_img is not None and (tuple(dy_img.shape) != tuple(dy.shape) or dy_img.stride() != dy.stride() or dy_img.dtype != torch.bfloat16):
        raise ValueError("speechsplit_amd: dy_img must be a bfloat16 view with dy's shape and strides")
    if part is not None:
        assert part.is_contiguous() and part.numel() >= B * 3 * Cc
    _capi.check(_capi.lib().ss_op_gn_relu_bwd(xp, x_ld, x_bs, dp, d_ld, d_bs, _ptr(gamma), _ptr(beta), _ptr(stats), _ptr(g_gamma), _ptr(g_beta),
                                              _ptr(g_bias), _ptr(amax), _ptr(part), _ptr(lam), _ptr(start), P, sp, s_ld, s_bs, _ptr(dy_img), B, T, Cc,
                                              _stream()))
    return dy


def _slab(x):
    """[B,T,C] -> haloed slab [B,T+4,C] (kernels.h: frame t at row t+2, zero halo rows)."""
    B, T, Cc = x.shape
    s = torch.zeros(B, T + 4, Cc, device=x.device)
    s[:, 2:2 + T] = x
    return s


def lstm_wgrad_scratch(H, In):
    """Scratch floats ss_op_lstm_wgrad needs (include/speechsplit_amd.h): 16 * 4096 * tiles partial slabs + one arrival counter per tile,
    rounded up to 64."""
    tiles = ((8 * H + 63) // 64) * ((In + 63) // 64 + (1 if (4 * H) % 64 == 0 else 2))
    return 16 * 4096 * tiles + (tiles + 63) // 64 * 64


def lstm_wgrad(dg, x, hout, scratch=None, out=None):
    """Test hook (ss_op_lstm_wgrad): the fused weight / bias gradient kernel of the encoder BLSTMs.  dg [R, 8H], x [R, In] (may be a
    column view of a wider tensor), hout [R, 2H] -> (gw_ih [2, 4H, In], gw_hh [2, 4H, H], gb [2, 2, 4H]).  scratch: pre-placed, at least
    lstm_wgrad_scratch(H, In) floats; out: pre-placed dense (gw_ih, gw_hh, gb), which the kernel ACCUMULATES into."""
    lib = _capi.lib()
    R, H8 = dg.shape
    H, In = H8 // 8, x.shape[1]
    dev = dg.device
    if scratch is None:
        scratch = torch.empty(lstm_wgrad_scratch(H, In) + 256, device=dev)
    if out is None:
        out = torch.zeros(2, 4 * H, In, device=dev), torch.zeros(2, 4 * H, H, device=dev), torch.zeros(2, 2, 4 * H, device=dev)
    gwih, gwhh, gb = out
    assert dg.is_contiguous() and hout.is_contiguous() and x.stride(1) == 1 and all(t.is_contiguous() for t in out) and scratch.is_contiguous()
    _capi.check(lib.ss_op_lstm_wgrad(_ptr(dg), _ptr(x), x.stride(0), _ptr(hout), _ptr(gwih), _ptr(gwhh), _ptr(gb), _ptr(scratch), scratch.numel(), R, H, In,
                                     _stream()))
    return gwih, gwhh, gb


def _view3(t, name, dtype=torch.float32):
    """A [B, T, C] view with unit channel stride -> (pointer to frame 0 of utterance 0, ld, bs)."""
    if t.dim() != 3 or t.stride(2) != 1 or t.dtype != dtype:
        raise ValueError(f'speechsplit_amd: {name} must be a [B, T, C] view with unit channel stride, got {tuple(t.shape)}')
    return _ptr(t), t.stride(1), t.stride(0)


def mse_loss(out, tgt, d_out, partials, loss, grad_scale=1.0):
    """Test hook (ss_op_mse_loss): the MSE loss kernels on the caller's [B, T, C] views.  d_out is written, partials (>= 8 B floats) is
    scratch, loss one float."""
    B, T, Cc = out.shape
    assert tuple(tgt.shape) == (B, T, Cc) and tuple(d_out.shape) == (B, T, Cc) and partials.numel() >= 8 * B
    (op, o_ld, o_bs), (tp, t_ld, t_bs), (dp, d_ld, d_bs) = _view3(out, 'out'), _view3(tgt, 'tgt'), _view3(d_out, 'd_out')
    _capi.check(_capi.lib().ss_op_mse_loss(op, o_ld, o_bs, tp, t_ld, t_bs, dp, d_ld, d_bs, B, T, Cc, float(grad_scale), _ptr(partials), _ptr(loss),
                                           _stream()))
    return loss


def ce_loss(logits, tgt, d_out, partials, loss, grad_scale=1.0):
    """Test hook (ss_op_ce_loss): softmax cross-entropy on the caller's [B, T, C] views against tgt i32 [B, T] (dense).  The targets are
    asserted to lie in [0, C) here, on the host: the device does not check them."""
    B, T, Cc = logits.shape
    assert tuple(d_out.shape) == (B, T, Cc) and partials.numel() >= B * T
    if tgt.dtype != torch.int32 or tuple(tgt.shape) != (B, T) or not tgt.is_contiguous():
        raise ValueError('speechsplit_amd: tgt must be a contiguous i32 [B, T]')
    if int(tgt.min()) < 0 or int(tgt.max()) >= Cc:
        raise ValueError('speechsplit_amd: ce_loss: a target lies outside [0, C)')
    (lp, l_ld, l_bs), (dp, d_ld, d_bs) = _view3(logits, 'logits'), _view3(d_out, 'd_out')
    _capi.check(_capi.lib().ss_op_ce_loss(lp, l_ld, l_bs, _ptr(tgt), dp, d_ld, d_bs, B, T, Cc, float(grad_scale), _ptr(partials), _ptr(loss),
                                          _stream()))
    return loss


def colsum_scratch_doubles(cols):
    """float64 words of scratch the chunked column sum needs (ss_op_colsum_scratch_doubles)."""
    return int(_capi.lib().ss_op_colsum_scratch_doubles(cols))


def colsum(x, outs, two_dir=False, part=None, ctr=None):
    """Test hook (ss_op_colsum): column sums of x [R, cols] (a view, unit column stride) ADDED to outs: (o0,) with cols = C, or
    (o0, o1, o2, o3) with cols = 2 C (o1 / o3 may be None).  part (float64) / ctr (i32, zero): the chunked form's scratch."""
    R, cols = x.shape
    assert x.stride(1) == 1 and x.dtype == torch.float32
    outs = tuple(outs) + (None,) * (4 - len(outs))
    Cc = cols // 2 if two_dir else cols
    assert not two_dir or cols % 2 == 0
    assert all(o is None or (o.is_contiguous() and o.numel() >= Cc) for o in outs)
    assert part is None or part.dtype == torch.float64
    assert ctr is None or ctr.dtype == torch.int32
    _capi.check(_capi.lib().ss_op_colsum(_ptr(x), x.stride(0) if R > 1 else max(cols, x.stride(0)), R, Cc, 1 if two_dir else 0, *[_ptr(o) for o in outs],
                                         _ptr(part), part.numel() if part is not None else 0, _ptr(ctr), ctr.numel() if ctr is not None else 0,
                                         _stream()))
    return outs


def _code_srcs(srcs, B, T, grad):
    """[(slab view [B, T+4, 2H] with row stride ld and batch stride (T+4) ld, H, freq, col)] -> the ss_code_src array."""
    arr = (_capi.SSCodeSrc * len(srcs))()
    for i, (t, H, freq, col) in enumerate(srcs):
        if tuple(t.shape) != (B, T + 4, 2 * H) or t.stride(2) != 1 or t.dtype != torch.float32 or (B > 1 and t.stride(0) != (T + 4) * t.stride(1)):
            raise ValueError(f'speechsplit_amd: source {i} must be a float32 slab view [B, T + 4, 2H] whose utterances follow each other')
        arr[i] = _capi.SSCodeSrc(None if grad else t.data_ptr(), t.data_ptr() if grad else None, H, freq, col, t.stride(1))
    return arr


def dec_in(srcs, emb, emb_col, dst, T, f=0, via_codes=None):
    """Test hook (ss_op_dec_in): the decoder input from encoder BLSTM output slabs srcs = [(o, H, freq, col)] and speaker rows emb [B, E]
    (None: no speaker columns) into dst: [B, T+4, ld] contiguous (f == 0, halo rows untouched) or [B, T/f, ld] (f > 0, the compact form).
    via_codes: a float32 scratch tensor -- go through dense codes instead (ss_op_dec_in_codes: export_codes, then dec_in_from_codes)."""
    B, rows, ld = dst.shape
    assert dst.is_contiguous() and rows == (T // f if f else T + 4)
    E = 0 if emb is None else emb.shape[1]
    assert emb is None or (emb.is_contiguous() and emb.shape[0] == B)
    arr = _code_srcs(srcs, B, T, False)
    if via_codes is not None:
        _capi.check(_capi.lib().ss_op_dec_in_codes(arr, len(srcs), _ptr(emb), E, emb_col, _ptr(via_codes), via_codes.numel(), _ptr(dst), ld, B, T, f,
                                                   _stream()))
    else:
        _capi.check(_capi.lib().ss_op_dec_in(arr, len(srcs), _ptr(emb), E, emb_col, _ptr(dst), ld, B, T, f, _stream()))
    return dst


def dec_in_grad(srcs, d_in, T, f=0):
    """Test hook (ss_op_dec_in_grad): the adjoint of dec_in.  srcs = [(d_o, H, freq, col)], the gradient slabs written (real columns of
    real rows only); d_in [B, T+4, ld] contiguous (f == 0) or the block sums [B, T/f, ld] (f > 0)."""
    B, rows, ld = d_in.shape
    assert d_in.is_contiguous() and rows == (T // f if f else T + 4)
    arr = _code_srcs(srcs, B, T, True)
    _capi.check(_capi.lib().ss_op_dec_in_grad(arr, len(srcs), _ptr(d_in), ld, B, T, f, _stream()))


def dec_in_codes_grad(codes, d_in, T, f=0):
    """Test hook (ss_op_dec_in_codes_grad): the adjoint of the decoder input with respect to DENSE codes, as ss_*_decode_backward runs it.
    codes = [(d_code, H, freq, col)], d_code [B, T/freq, 2H] contiguous float32 and written whole; d_in [B, T+4, ld] (f == 0; a view with
    unit column stride whose utterances follow each other) or the block sums [B, T/f, ld] (f > 0).  One launch for up to three codes."""
    B, rows, _ = d_in.shape
    ld = d_in.stride(1)
    assert d_in.stride(2) == 1 and rows == (T // f if f else T + 4) and (B == 1 or d_in.stride(0) == rows * ld)
    arr = (_capi.SSCodeSrc * len(codes))()
    for i, (t, H, freq, col) in enumerate(codes):
        if tuple(t.shape) != (B, T // freq, 2 * H) or not t.is_contiguous() or t.dtype != torch.float32:
            raise ValueError(f'speechsplit_amd: code gradient {i} must be a contiguous float32 [B, T / freq, 2H]')
        arr[i] = _capi.SSCodeSrc(None, t.data_ptr(), H, freq, col, 2 * H)
    _capi.check(_capi.lib().ss_op_dec_in_codes_grad(arr, len(codes), _ptr(d_in), ld, B, T, f, _stream()))


def spk_grad(dg, w_f, w_r, col0, E, out):
    """Test hook (ss_op_spk_grad): the speaker-embedding contraction.  dg [B, rows, 2 H4] (a view), w_f / w_r [H4, >= col0 + E] (views),
    out [B, E] contiguous: out[b] = (sum over rows of dg[b]) . [w_f ; w_r][:, col0 : col0 + E]."""
    B, rows, G = dg.shape
    H4 = G // 2
    assert dg.stride(2) == 1 and w_f.stride(1) == 1 and w_r.stride(1) == 1 and w_f.stride(0) == w_r.stride(0) and w_f.shape[0] == H4 == w_r.shape[0]
    assert out.is_contiguous() and tuple(out.shape) == (B, E)
    _capi.check(_capi.lib().ss_op_spk_grad(_ptr(dg), dg.stride(1), dg.stride(0), rows, _ptr(w_f), _ptr(w_r), w_f.stride(0), col0, H4, E, _ptr(out), B,
                                           _stream()))
    return out


def _dp(t):
    return t.data_ptr() if t is not None else None


def _wgrad_tasks(tasks):
    """[(dg [R, 8H] contiguous, x [R, In] view, hout [R, 2H] view, gwih, gwhh, gb flat)] -> the ss_wgrad_task array"""
    arr = (_capi.SSWgradTask * len(tasks))()
    for i, (dg, x, hout, gwih, gwhh, gb) in enumerate(tasks):
        R, In = x.shape
        H = hout.shape[1] // 2
        if tuple(dg.shape) != (R, 8 * H) or not dg.is_contiguous() or hout.shape[0] != R or x.stride(1) != 1 or hout.stride(1) != 1:
            raise ValueError(f'speechsplit_amd: wgrad task {i}: dg must be a contiguous [R, 8H], x [R, In] and hout [R, 2H] views with unit column stride')
        if gwih.numel() != 8 * H * In or gwhh.numel() != 8 * H * H or gb.numel() != 16 * H:
            raise ValueError(f'speechsplit_amd: wgrad task {i}: gwih / gwhh / gb must hold [2, 4H, In] / [2, 4H, H] / [2, 2, 4H] floats')
        arr[i] = _capi.SSWgradTask(dg.data_ptr(), x.data_ptr(), x.stride(0) if R > 1 else max(In, x.stride(0)), hout.data_ptr(),
                                   hout.stride(0) if R > 1 else max(2 * H, hout.stride(0)), gwih.data_ptr(), gwhh.data_ptr(), gb.data_ptr(), H, In, R)
    return arr


def lstm_wgrad_table_sizes(tasks, row_groups):
    """(floats of scratch, counter words) an lstm_wgrad_table launch of these tasks needs"""
    arr = _wgrad_tasks(tasks)
    return (int(_capi.lib().ss_op_lstm_wgrad_table_floats(arr, len(tasks), row_groups)), int(_capi.lib().ss_op_lstm_wgrad_table_counters(arr, len(tasks))))


def lstm_wgrad_table(tasks, row_groups, part, ctr):
    """Test hook (ss_op_lstm_wgrad_table): the fused encoder-BLSTM weight gradients of up to eight tasks in one launch, ADDED to each task's
    gwih / gwhh / gb.  part: float32 scratch, ctr: i32 counters, zero on entry (zero again afterwards)."""
    assert part.dtype == torch.float32 and ctr.dtype == torch.int32 and part.is_contiguous() and ctr.is_contiguous()
    _capi.check(_capi.lib().ss_op_lstm_wgrad_table(_wgrad_tasks(tasks), len(tasks), row_groups, _ptr(part), part.numel(), _ptr(ctr), ctr.numel(), _stream()))


def _words(t, dtype, n, name):
    if t.dtype != dtype or not t.is_contiguous() or t.numel() != n:
        raise ValueError(f'speechsplit_amd: {name} must be a contiguous {dtype} tensor of {n} elements')
    return _ptr(t)


def interp_plan(scales, len_seg, len_seq, T, P, ncand, i0, lam, nrows, counts, start):
    """Test hook (ss_op_interp_plan): the resampling plan of B utterances from their draws.  scales f32 [B, S], len_seg i32 [B, S], len_seq
    i32 [B] (or an int: every utterance's length) -> i0 i32 [B, P], lam f32 [B, P], nrows / counts i32 [B], start i32 [B, T + 1], all given."""
    B, S = scales.shape
    const = isinstance(len_seq, int)
    i32, f32 = torch.int32, torch.float32
    _capi.check(_capi.lib().ss_op_interp_plan(
        _words(scales, f32, B * S, 'scales'), _words(len_seg, i32, B * S, 'len_seg'), _ptr(None) if const else _words(len_seq, i32, B, 'len_seq'),
        len_seq if const else 0, S, ncand, P, T, B, _words(i0, i32, B * P, 'i0'), _words(lam, f32, B * P, 'lam'), _words(nrows, i32, B, 'nrows'),
        _words(counts, i32, B, 'counts'), _words(start, i32, B * (T + 1), 'start'), _stream()))


def interp_gather(i0, lam, nrows, x, y, y_img=None, img_scale=None):
    """Test hook (ss_op_interp_gather): y [B, P, C] = the resampled x [B, T, C] (views, frame 0 first); y_img: a view with y's strides."""
    B, P = i0.shape
    Cc = x.shape[2]
    assert tuple(y.shape) == (B, P, Cc) and x.shape[0] == B
    (xp, x_ld, x_bs), (yp, y_ld, y_bs) = _view3(x, 'x'), _view3(y, 'y')
    assert y_img is None or (y_img.stride() == y.stride() and tuple(y_img.shape) == tuple(y.shape))
    i32, f32 = torch.int32, torch.float32
    _capi.check(_capi.lib().ss_op_interp_gather(_words(i0, i32, B * P, 'i0'), _words(lam, f32, B * P, 'lam'), _words(nrows, i32, B, 'nrows'), P, xp, x_ld,
                                                x_bs, yp, y_ld, y_bs, Cc, B, _ptr(y_img), _ptr(img_scale), _stream()))
    return y


def interp_quant(i0, lam, nrows, mel, f0, ymel, yoh, noh, qidx):
    """Test hook (ss_op_interp_quant): mel [B, T, CM] and f0 [B, T] contiguous -> ymel [B, P, CM] (a view), yoh [B, P, yo_ld] (a view whose
    row stride is its width: every column of the row is written) and qidx i32 [B, P]."""
    B, P = i0.shape
    T, CM = mel.shape[1], mel.shape[2]
    assert mel.is_contiguous() and f0.is_contiguous() and tuple(f0.shape) == (B, T) and tuple(ymel.shape) == (B, P, CM)
    assert tuple(yoh.shape[:2]) == (B, P) and yoh.stride(1) == yoh.shape[2]
    (mp, m_ld, m_bs), (op, o_ld, o_bs) = _view3(ymel, 'ymel'), _view3(yoh, 'yoh')
    i32, f32 = torch.int32, torch.float32
    _capi.check(_capi.lib().ss_op_interp_quant(_words(i0, i32, B * P, 'i0'), _words(lam, f32, B * P, 'lam'), _words(nrows, i32, B, 'nrows'), P, T,
                                               _ptr(mel), _ptr(f0), CM, mp, m_ld, m_bs, op, o_ld, o_bs, noh, _words(qidx, i32, B * P, 'qidx'), B,
                                               _stream()))


def interp_scatter(lam, start, dy, dx):
    """Test hook (ss_op_interp_scatter): dx [B, T, C] = the adjoint of interp_gather applied to dy [B, P, C] (views)."""
    B, P = lam.shape
    T, Cc = dx.shape[1], dx.shape[2]
    assert tuple(dy.shape) == (B, P, Cc) and dx.shape[0] == B
    (yp, y_ld, y_bs), (xp, x_ld, x_bs) = _view3(dy, 'dy'), _view3(dx, 'dx')
    _capi.check(_capi.lib().ss_op_interp_scatter(_words(lam, torch.float32, B * P, 'lam'), _words(start, torch.int32, B * (T + 1), 'start'), P, T, yp,
                                                 y_ld, y_bs, xp, x_ld, x_bs, Cc, B, _stream()))
    return dx


def conv_pack(w, Cp, wf, wb=None, wf_img=None, wb_img=None, img_bf16=False):
    """Test hook (ss_op_conv_pack): w [Co, Ci, 5] contiguous -> wf [Co, 5, Cp] (+ wb [Ci, 5, Co], + their images), all flat device tensors."""
    Co, Ci, K = w.shape
    assert K == 5 and w.is_contiguous() and w.dtype == torch.float32
    _capi.check(_capi.lib().ss_op_conv_pack(_ptr(w), Co, Ci, Cp, _ptr(wf), _ptr(wb), _ptr(wf_img), _ptr(wb_img), 1 if img_bf16 else 0, _stream()))


def conv_pack_many(tasks, img_bf16=False):
    """Test hook (ss_op_conv_pack_many): tasks = [(w, Cp, wf, wb, wf_img, wb_img)] as conv_pack's arguments, one launch."""
    arr = (_capi.SSConvPackTask * len(tasks))()
    for i, (w, Cp, wf, wb, wf_img, wb_img) in enumerate(tasks):
        Co, Ci, K = w.shape
        assert K == 5 and w.is_contiguous() and w.dtype == torch.float32
        arr[i] = _capi.SSConvPackTask(_dp(w), _dp(wf), _dp(wb), _dp(wf_img), _dp(wb_img), Co, Ci, Cp)
    _capi.check(_capi.lib().ss_op_conv_pack_many(arr, len(tasks), 1 if img_bf16 else 0, _stream()))


def conv_pack_dx(w, wb):
    """Test hook (ss_op_conv_pack_dx): w [Co, Ci, 5] contiguous -> wb [Ci, 5, Co], any Ci and Co."""
    Co, Ci, K = w.shape
    assert K == 5 and w.is_contiguous() and w.dtype == torch.float32
    _capi.check(_capi.lib().ss_op_conv_pack_dx(_ptr(w), Co, Ci, _ptr(wb), _stream()))


def conv_unpack(gp, Co, Ci, Cp, g, acc=False):
    """Test hook (ss_op_conv_unpack): packed gradient gp [Co, 5, Cp] -> g [Co, Ci, 5] (acc: added to g), flat device tensors."""
    _capi.check(_capi.lib().ss_op_conv_unpack(_ptr(gp), Co, Ci, Cp, _ptr(g), 1 if acc else 0, _stream()))


def conv_unpack_many(tasks, acc=False):
    """Test hook (ss_op_conv_unpack_many): tasks = [(gp, Co, Ci, Cp, g)], one launch."""
    arr = (_capi.SSConvUnpackTask * len(tasks))()
    for i, (gp, Co, Ci, Cp, g) in enumerate(tasks):
        arr[i] = _capi.SSConvUnpackTask(_dp(gp), _dp(g), Co, Ci, Cp)
    _capi.check(_capi.lib().ss_op_conv_unpack_many(arr, len(tasks), 1 if acc else 0, _stream()))


def prep(tasks, img_bf16=False):
    """Test hook (ss_op_prep): tasks = [(a, b or None, dst, n, img or None)] over flat device tensors: dst[:n] = a[:n] + b[:n], or a copy."""
    arr = (_capi.SSPrepTask * len(tasks))()
    for i, (a, b, dst, n, img) in enumerate(tasks):
        arr[i] = _capi.SSPrepTask(_dp(a), _dp(b), _dp(dst), n, _dp(img))
    _capi.check(_capi.lib().ss_op_prep(arr, len(tasks), 1 if img_bf16 else 0, _stream()))


def transpose(x, out):
    """Test hook (ss_op_transpose): out [C, R] = x [R, C]^T, both contiguous."""
    R, Cc = x.shape
    assert x.is_contiguous() and out.is_contiguous() and out.numel() == R * Cc and x.dtype == torch.float32
    _capi.check(_capi.lib().ss_op_transpose(_ptr(x), R, Cc, _ptr(out), _stream()))
    return out


def copy_rows(src, dst, lengths=None):
    """Test hook (ss_op_copy_rows): dst[b, t, :] = src[b, t, :] over [B, T, C] views (frame 0 first; a slab is passed as slab[:, 2:2 + T]);
    lengths (i32 [B] on the device): zeros at and beyond each row's length, whose source rows are not read."""
    B, T, Cc = src.shape
    assert tuple(dst.shape) == (B, T, Cc) and (lengths is None or (lengths.dtype == torch.int32 and lengths.numel() == B))
    (sp, s_ld, s_bs), (dp, d_ld, d_bs) = _view3(src, 'src'), _view3(dst, 'dst')
    _capi.check(_capi.lib().ss_op_copy_rows(sp, s_ld, s_bs, dp, d_ld, d_bs, _ptr(lengths), B, T, Cc, _stream()))
    return dst


def act_scales(affines, T, out):
    """Test hook (ss_op_act_scales): affines = [(gamma, beta)] (1-D views of equal length, or (None, None) for an absent block) -> out[i]."""
    n = len(affines)
    g = (C.c_void_p * n)(*[_dp(a) for a, _ in affines])
    b = (C.c_void_p * n)(*[_dp(a) for _, a in affines])
    cs = (C.c_int * n)(*[0 if a is None else a.numel() for a, _ in affines])
    assert all(a is None or (a.stride(0) == 1 and bb.stride(0) == 1 and a.numel() == bb.numel()) for a, bb in affines) and out.numel() >= n
    _capi.check(_capi.lib().ss_op_act_scales(g, b, cs, n, T, _ptr(out), _stream()))
    return out


def param_guard(p, limit, sticky):
    """Test hook (ss_op_param_guard): sticky (one i32 word) |= 4 if an element of the flat p is not finite or has |p| >= limit."""
    assert p.dtype == torch.float32 and p.dim() == 1 and p.stride(0) == 1 and sticky.dtype == torch.int32
    _capi.check(_capi.lib().ss_op_param_guard(_ptr(p), p.numel(), float(limit), _ptr(sticky), _stream()))
    return sticky


def small_lstm_ld(H):
    """Row stride of the output / cell-state / output-gradient slabs of a BLSTM layer (kernels.h lstm_small_ld): 2H, rounded up to a
    multiple of 4 floats when H <= 32 is not a power of two."""
    return 2 * H if H > 32 or H & (H - 1) == 0 else (2 * H + 3) // 4 * 4


def lstm_scratch(B, H, backward, persist=True):
    """Scratch floats ss_op_lstm_fwd / ss_op_lstm_bwd need, by the header's formulas (include/speechsplit_amd.h): none for H <= 32; else
    8 H^2 + 4 ceil16(B) H (forward) or 8 H^2 + 16 ceil16(B) H + 2 B H (backward), and for the backward as ONE persistent launch
    (H in {256, 512}) at least its exchange tiles and flags, 4 ceil(B / 16) (H / 16)^2 * 1024 + 8192 bytes."""
    if H <= 32:
        return 0
    B16 = (B + 15) // 16 * 16
    if not backward:
        return 8 * H * H + 4 * B16 * H
    n = 8 * H * H + 16 * B16 * H + 2 * B * H
    if persist and H in (256, 512):
        n = max(n, (4 * (B16 // 16) * (H // 16) ** 2 * 1024 + 8192) // 4)
    return n


def _blstm_recurrence_slabs(gates_real, w_hh, d_out, lengths, place, want_act, seq=None):
    """The recurrences of one BLSTM layer on haloed slabs: gates_real [B,T,8H] pre-activations -> (gates, out, csave, act) with gates
    [R,8H] holding the activated gates (no d_out) or the pre-activation gradients (d_out given), out / csave [B,T+4,ld] and act a clone
    of the real frames' activated gates taken before the backward overwrites them (want_act only, else None).
    seq (seq_recurrence): the option pointers of ss_op_lstm_seq_fwd / _bwd, which then run in the place of ss_op_lstm_fwd / _bwd."""
    lib = _capi.lib()
    B, T, H8 = gates_real.shape
    H = w_hh[0].shape[1]
    assert H8 == 8 * H
    OW = small_lstm_ld(H)                                                   # row stride of out / csave / d_out
    dev = gates_real.device
    R = B * (T + 4)
    gates = torch.zeros(R, 8 * H, device=dev) if place is None else place('gates', (R, 8 * H))
    gates.view(B, T + 4, 8 * H)[:, 2:2 + T] = gates_real
    gates.view(B, T + 4, 8 * H)[:, :2] = 0
    gates.view(B, T + 4, 8 * H)[:, T + 2:] = 0
    B16 = (B + 15) // 16 * 16
    if place is None:
        out = torch.zeros(B, T + 4, OW, device=dev)
        csave = torch.zeros(B, T + 4, OW, device=dev)
        nscr = 8 * H * H + 16 * B16 * H + 2 * B * H + (4 * ((B + 15) // 16) * (H // 16) ** 2 * 1024 + 8192) // 4 + 4096
        scratch = scratch_b = torch.zeros(max(nscr, 1), device=dev)
    else:
        out, csave = place('out', (B, T + 4, OW)), place('csave', (B, T + 4, OW))
        scratch = place('scratch_fwd', (max(lstm_scratch(B, H, False), 1),))
        scratch_b = place('scratch_bwd', (max(lstm_scratch(B, H, True), 1),)) if d_out is not None else None
        for t in (gates, out, csave, scratch):
            assert t.is_contiguous()
    whf, whb = w_hh[0].contiguous(), w_hh[1].contiguous()
    real = lambda: gates.view(B, T + 4, 8 * H)[:, 2:2 + T].clone()
    if lengths is not None and d_out is not None:
        raise ValueError('speechsplit_amd: a ragged BLSTM layer runs the forward only')
    if seq is not None:
        ln = None if lengths is None else check_lengths(lengths, B, T, (1,), dev)
        _capi.check(lib.ss_op_lstm_seq_fwd(_ptr(gates), _ptr(whf), _ptr(whb), _ptr(out), _ptr(csave), _ptr(scratch), scratch.numel(), _ptr(seq['xc']),
                                           int(seq['xf']), _ptr(seq['out_img']), int(seq['img_bf16']), int(seq['hi_only']), _ptr(ln), B, T, H, _stream()))
        act = real() if want_act else None
        if d_out is None:
            return gates, out, csave, act
        ds = _slab(d_out.to(dev))
        scratch_b.zero_()
        _capi.check(lib.ss_op_lstm_seq_bwd(_ptr(gates), _ptr(whf), _ptr(whb), _ptr(ds), _ptr(csave), _ptr(scratch_b), scratch_b.numel(),
                                           _ptr(seq['amax']), _ptr(seq['gbias_f']), _ptr(seq['gbias_b']), _ptr(seq['dgs']), int(seq['xf']),
                                           _ptr(seq['dimg']), int(seq['img_only']), int(seq['hi_only']), B, T, H, _stream()))
        return gates, out, csave, act
    if lengths is not None:
        ln = check_lengths(lengths, B, T, (1,), dev)
        _capi.check(lib.ss_op_lstm_fwd_ragged(_ptr(gates), _ptr(whf), _ptr(whb), _ptr(out), _ptr(csave), _ptr(scratch), scratch.numel(),
                                              _ptr(ln), B, T, H, _stream()))
        return gates, out, csave, real() if want_act else None
    _capi.check(lib.ss_op_lstm_fwd(_ptr(gates), _ptr(whf), _ptr(whb), _ptr(out), _ptr(csave), _ptr(scratch), scratch.numel(),
                                   B, T, H, _stream()))
    act = real() if want_act else None
    if d_out is None:
        return gates, out, csave, act
    if place is None:
        ds = _slab(torch.nn.functional.pad(d_out.to(dev), (0, OW - 2 * H)))
        scratch_b.zero_()
    else:
        ds = place('d_out', (B, T + 4, OW))
        assert ds.is_contiguous() and scratch_b.is_contiguous()
        ds[:, 2:2 + T, :2 * H] = d_out.to(dev)
    _capi.check(lib.ss_op_lstm_bwd(_ptr(gates), _ptr(whf), _ptr(whb), _ptr(ds), _ptr(csave), _ptr(scratch_b), scratch_b.numel(),
                                   B, T, H, _stream()))
    return gates, out, csave, act


def blstm_recurrence(gates, w_hh, d_out=None, lengths=None, place=None):
    """Test hook: the recurrences of one bidirectional LSTM layer (ss_op_lstm_fwd / _ragged, and with d_out ss_op_lstm_bwd) on the CALLER's
    pre-activations.  gates [B,T,8H]: x.W_ih^T + b of the forward direction in columns [0,4H), of the reverse direction in [4H,8H), gate
    order i, f, g, o; w_hh: (forward, reverse) [4H,H].  Returns (out [B,T,2H], csave [B,T,2H], act [B,T,8H], dgates [B,T,8H] or None),
    halo rows stripped: act is what the forward left in the gates slab (the activated gates), copied before the backward replaces it by the
    pre-activation gradients dgates.  lengths: a ragged batch (forward only): out / csave are zero and act is unspecified at t >= lengths[b].
    place: as for blstm_layer."""
    B, T, H8 = gates.shape
    H = H8 // 8
    slab, out, csave, act = _blstm_recurrence_slabs(gates.to(dtype=torch.float32), w_hh, d_out, lengths, place, True)
    dgates = slab.view(B, T + 4, 8 * H)[:, 2:2 + T].clone() if d_out is not None else None
    return out[:, 2:2 + T, :2 * H].clone(), csave[:, 2:2 + T, :2 * H].clone(), act, dgates


SEQ_GUARD = 4096          # bytes of guard region behind every side output seq_recurrence returns, beside the padded utterances' room
SEQ_FILL = 0xA5           # the byte those guards and the images are pre-filled with


def seq_recurrence(pre_or_xc, w_hh, d_out=None, *, xf=0, out_img=None, hi_only=False, lengths=None, amax0=None, gbias0=None, dgs=False,
                   dimg=False, img_only=False):
    """Test hook (ss_op_lstm_seq_fwd / _bwd): the persistent recurrences (H in {256, 512}) launched with the options the engine passes them;
    no fall-back, what the persistent kernels cannot run raises.  pre_or_xc: the pre-activations [B,T,8H], or with xf > 0 their compact
    form [B,T/xf,8H] (the input repeats in blocks of xf frames) -- the gates slab then starts with NaN in every real row, which the kernel
    only writes.  out_img: 'v2' or 'bf16'; amax0: the start value of the amax word; gbias0 [8H]: start value of both halves (b_ih, b_hh)
    of the bias-gradient accumulators, forward direction in [0,4H); dgs / dimg / img_only: SeqBwd's (dgs sums per block of xf frames, xf = 0:
    of one frame).  Returns a dict: out, csave, act, dgates as blstm_recurrence returns them (dgates: the real rows of the gates slab after the
    backward, so under img_only the activated gates it kept) and every requested side output as a RAW uint8 tensor with a guard region of
    SEQ_FILL behind it -- for the per-utterance outputs (out_img, dimg, dgs) the room the 16 ceil(B/16) - B padded utterances of the last batch
    tile would take, then SEQ_GUARD bytes; SEQ_GUARD bytes for amax and gbias: out_img / dimg over the whole haloed slab ([B,T+4,2H] / [B,T+4,8H] elements of 4 bytes (v2) or 2 (bf16), pre-filled
    with SEQ_FILL), amax (4 bytes), gbias ([2 directions][2 halves][4H] floats), dgs ([B,T/xf,8H] floats, pre-filled with NaN)."""
    pre_or_xc = pre_or_xc.to(dtype=torch.float32).contiguous()
    dev = pre_or_xc.device
    B, Tc, H8 = pre_or_xc.shape
    H = H8 // 8
    T = Tc * xf if xf > 0 else Tc
    bxf = xf if xf > 0 else 1
    if out_img not in (None, 'v2', 'bf16'):
        raise ValueError("speechsplit_amd: out_img is None, 'v2' or 'bf16'")

    pad = (B + 15) // 16 * 16 - B                            # utterances a kernel that lost its b < B test would also write

    def raw(nbytes, fill=None, per_utt=0):
        t = torch.full((nbytes + pad * per_utt + SEQ_GUARD,), SEQ_FILL, dtype=torch.uint8, device=dev)
        if fill is not None:
            t[:nbytes].view(torch.float32).copy_(fill.reshape(-1))
        return t
    side = {}
    if out_img:
        side['out_img'] = raw(B * (T + 4) * 2 * H * (4 if out_img == 'v2' else 2), None, (T + 4) * 2 * H * (4 if out_img == 'v2' else 2))
    if d_out is not None:
        if amax0 is not None:
            side['amax'] = raw(4, torch.tensor([float(amax0)], device=dev))
        if gbias0 is not None:
            g0 = torch.as_tensor(gbias0, dtype=torch.float32, device=dev).view(2, 1, 4 * H).expand(2, 2, 4 * H).contiguous()
            side['gbias'] = raw(4 * 16 * H, g0)
        if dgs:
            side['dgs'] = raw(4 * B * (T // bxf) * 8 * H, torch.full((B * (T // bxf) * 8 * H,), float('nan'), device=dev), 4 * (T // bxf) * 8 * H)
        if dimg:
            side['dimg'] = raw(2 * B * (T + 4) * 8 * H, None, 2 * (T + 4) * 8 * H)
    fl = lambda name, off=0: side[name][off:].view(torch.float32) if name in side else None
    seq = dict(xc=pre_or_xc if xf > 0 else None, xf=bxf if (xf > 0 or dgs) else 0, out_img=fl('out_img'), img_bf16=out_img == 'bf16',
               hi_only=hi_only, amax=fl('amax'), gbias_f=fl('gbias'), gbias_b=fl('gbias', 4 * 8 * H), dgs=fl('dgs'), dimg=fl('dimg'), img_only=img_only)
    gates_real = torch.full((B, T, 8 * H), float('nan'), device=dev) if xf > 0 else pre_or_xc
    slab, out, csave, act = _blstm_recurrence_slabs(gates_real, w_hh, d_out, lengths, None, True, seq)
    res = dict(out=out[:, 2:2 + T, :2 * H].clone(), csave=csave[:, 2:2 + T, :2 * H].clone(), act=act,
               dgates=slab.view(B, T + 4, 8 * H)[:, 2:2 + T].clone() if d_out is not None else None)
    res.update(side)
    return res


def blstm_layer(x, w_ih, w_hh, b_ih, b_hh, d_out=None, place=None, lengths=None):
    """Test hook: one bidirectional LSTM layer through ss_op_lstm_fwd / ss_op_lstm_bwd (the engine's recurrence kernels) with
    the input projection and the weight / input gradients on the engine's GEMM (ss_op_gemm): the projection, then the recurrences as
    blstm_recurrence runs them, then the gradient GEMMs.  w_ih etc. are (forward, reverse)
    pairs with PyTorch's shapes.  Returns out [B,T,2H]; with d_out also (dx, [(gw_ih, gw_hh, gb) per direction]).
    place(name, shape): optional allocator of the recurrences' operands -- 'gates' [R,8H], 'out' / 'csave' / 'd_out' [B,T+4,ld] and
    'scratch_fwd' / 'scratch_bwd' [lstm_scratch(...) floats, at least 1] -- for callers that pre-place them.  It returns a dense tensor that
    the CALLER has initialised as the kernels' contracts ask (halo rows of out / csave / d_out zero, scratch of a persistent recurrence
    zero); the hook fills gates entirely and the real frames' 2H columns of d_out, nothing else.
    lengths: per-row frame counts of a ragged batch (ss_op_lstm_fwd_ragged; forward only): out[b, lengths[b]:] comes back as zeros."""
    B, T, In = x.shape
    H = w_hh[0].shape[1]
    OW = small_lstm_ld(H)                                                   # row stride of out / csave / d_out
    dev = x.device
    wcat = torch.cat([w_ih[0], w_ih[1]], 0).contiguous()                    # [8H, In]
    bsum = torch.cat([b_ih[0] + b_hh[0], b_ih[1] + b_hh[1]]).contiguous()
    xs = _slab(x)
    R = B * (T + 4)
    g_real = gemm(xs.view(R, In), wcat, bsum)                               # all rows; the recurrence hook takes the real frames
    gates, out, csave, _ = _blstm_recurrence_slabs(g_real.view(B, T + 4, 8 * H)[:, 2:2 + T], w_hh, d_out, lengths, place, False)
    y = out[:, 2:2 + T, :2 * H].clone()
    if d_out is None:
        return y
    dG = gates.view(R, 8 * H)                                               # pre-activation gradients, halo rows zero
    dx = gemm(dG, wcat, tb=True).view(B, T + 4, In)[:, 2:2 + T].clone()     # dX = dG . W_ih (both directions)
    grads = []
    flat_x = xs.view(R, In)
    flat_o = out.view(R, OW)
    for d in range(2):
        dGd = dG[:, d * 4 * H:(d + 1) * 4 * H].contiguous()
        gw_ih = gemm(dGd, flat_x, ta=True, tb=True)                         # [4H, In] = dG^T . X
        hprev = torch.zeros(R, H, device=dev)
        if d == 0:
            hprev[1:] = flat_o[:-1, :H]                                     # forward: h(t-1) is one slab row earlier
        else:
            hprev[:-1] = flat_o[1:, H:2 * H]
        gw_hh = gemm(dGd, hprev, ta=True, tb=True)
        grads.append((gw_ih, gw_hh, dGd.sum(0)))
    return y, dx, grads


def tune(key, value):
    """Process-global tuning knob of the HIP library (ss_tune in include/speechsplit_amd.h)."""
    _capi.check(_capi.lib().ss_tune(key.encode(), int(value)))


def last_variant(what):
    """The kernel instance the last launch of kind 'gemm', 'lstm_step_fwd' or 'lstm_step_bwd' picked, as text (ss_debug_last_variant): a
    host-side record, so a test that sets a knob can prove which instance ran."""
    buf = C.create_string_buffer(8192)
    if _capi.lib().ss_debug_last_variant(what.encode(), buf, len(buf)) < 0:
        raise ValueError(_capi.lib().ss_last_error().decode())
    return buf.value.decode()


def seen_variants(what):
    """Every distinct instance of that kind launched since reset_variants(), in order of first appearance (ss_debug_last_variant("<kind>_seen"))."""
    return last_variant(what + '_seen').splitlines()


def reset_variants():
    """Forget the records: what last_variant / seen_variants return afterwards was written by launches made afterwards."""
    last_variant('reset')


def gemm(a, b, bias=None, ta=False, tb=False, ksplit=1, out=None, bf16=False, f16x2=False, a_img=None, b_img=None, part=None, as_engine=False):
    """Test hook for the MFMA GEMM: C[M,N] = A(m,k) B(n,k) (+bias).  a: [M,K] or [K,M] if ta; b: [N,K] or [K,N] if tb.
    as_engine (f16x2 only, ss_op_gemm_pre): the launch as the engine's weight gradients make it -- the largest tile the shape admits, the
    operands' images a_img / b_img (split_image, same strides as a / b) where given, and for ksplit > 1 partial slabs in `part`
    (ksplit * M * N floats) added in a fixed order instead of atomics."""
    lib = _capi.lib()
    M = a.shape[1] if ta else a.shape[0]
    K = a.shape[0] if ta else a.shape[1]
    N = b.shape[1] if tb else b.shape[0]
    assert (b.shape[0] if tb else b.shape[1]) == K
    c = torch.zeros(M, N, device=a.device) if out is None else out
    assert tuple(c.shape) == (M, N) and c.stride(1) == 1
    if as_engine:
        assert f16x2 and not bf16 and bias is None
        assert a_img is None or (a_img.shape == a.shape and a_img.stride() == a.stride())
        assert b_img is None or (b_img.shape == b.shape and b_img.stride() == b.stride())
        assert part is None or part.numel() >= ksplit * M * N
        _capi.check(lib.ss_op_gemm_pre(_ptr(a), a.stride(0), _ptr(a_img), _ptr(b), b.stride(0), _ptr(b_img), _ptr(c), c.stride(0), _ptr(part), M, N, K,
                                       (1 if ta else 0) | (2 if tb else 0), ksplit, _stream()))
        return c
    assert a_img is None and b_img is None and part is None
    _capi.check(lib.ss_op_gemm(_ptr(a), a.stride(0), _ptr(b), b.stride(0), _ptr(c), c.stride(0), _ptr(bias), M, N, K,
                               (1 if ta else 0) | (2 if tb else 0) | (8 if bf16 else 0) | (16 if f16x2 else 0), ksplit, _stream()))
    return c


def _at(buf, off):
    """Device address of element `off` of the flat buffer `buf` (None: null)."""
    return None if buf is None else buf.data_ptr() + int(off) * buf.element_size()


def _geom(g):
    """Operand geometry (off, ld, bstride=0, seglen=0, segstride=0), all in elements."""
    g = tuple(int(v) for v in g)
    return g + (0,) * (5 - len(g))


def gemm_desc(a, a_geom, b, b_geom, c, c_geom, M, N, K, *, batch=1, ta=False, tb=False, accumulate=False, bf16=False, f16x2=False, bias=None,
              want=0, row_mask=(0, 0, 0, 0), ksplit=1, amax_a=None, amax_b=None, a_img=None, b_img=None, a_pre_scale=None, b_pre_scale=None,
              part=None):
    """Test hook (ss_op_gemm_desc): one launch_gemm call with every descriptor field a product launch sets.  a, b, c are FLAT buffers --
    segmented and batched operands overlap, so they have no tensor shape; a_geom / b_geom = (off, ld, bstride, seglen, segstride) and
    c_geom = (off, ldc, cstride) place the matrices in them, in elements.  a_img / b_img: flat image buffers of the same geometry;
    amax_* / *_pre_scale: one-element device tensors; row_mask = (period, off, lo, hi); part: batch * ksplit * M * N floats."""
    ao, lda, abs_, asl, ass = _geom(a_geom)
    bo, ldb, bbs, bsl, bss = _geom(b_geom)
    co, ldc, cs = _geom(c_geom)[:3]
    d = _capi.SSGemmDesc(a=_at(a, ao), b=_at(b, bo), c=_at(c, co), bias=_at(bias, 0), amax_a=_at(amax_a, 0), amax_b=_at(amax_b, 0), a_pre=_at(a_img, ao),
                         b_pre=_at(b_img, bo), a_pre_scale=_at(a_pre_scale, 0), b_pre_scale=_at(b_pre_scale, 0), part=_at(part, 0), lda=lda, a_bstride=abs_,
                         a_segstride=ass, ldb=ldb, b_bstride=bbs, b_segstride=bss, ldc=ldc, cstride=cs, a_seglen=asl, b_seglen=bsl, M=M, N=N, K=K,
                         batch=batch, flags=(1 if ta else 0) | (2 if tb else 0) | (4 if accumulate else 0) | (8 if bf16 else 0) | (16 if f16x2 else 0),
                         want=want, row_period=row_mask[0], row_off=row_mask[1], row_lo=row_mask[2], row_hi=row_mask[3], ksplit=ksplit)
    _capi.check(_capi.lib().ss_op_gemm_desc(C.byref(d), _stream()))
    return c


def gemm_img_desc(a_img, a_geom, b_img, b_geom, c, c_geom, M, N, K, *, batch=1, ta=False, tb=False, accumulate=False, bias=None,
                  row_mask=(0, 0, 0, 0), rm=(0, 0), ksplit=1, part=None, scale_a=None, scale_b=None, zeros=None, cfg=-1):
    """Test hook (ss_op_gemm_img_desc): one launch_gemm_img call.  Flat buffers and geometry as gemm_desc (offsets and strides in ELEMENTS of
    the underlying matrix); torch.bfloat16 image buffers select the single-piece form.  rm = (rm_T, rm_TP); scale_a / scale_b: one-element
    device tensors (None: 16); zeros: >= 1 KB of zero bytes (None: a shared buffer)."""
    bf16 = a_img.dtype == torch.bfloat16
    assert (b_img.dtype == torch.bfloat16) == bf16
    ao, lda, abs_, asl, ass = _geom(a_geom)
    bo, ldb, bbs, bsl, bss = _geom(b_geom)
    co, ldc, cs = _geom(c_geom)[:3]
    z = _ZEROS.setdefault(str(c.device), torch.zeros(1024, device=c.device)) if zeros is None else zeros
    d = _capi.SSGemmImgDesc(a=_at(a_img, ao), b=_at(b_img, bo), c=_at(c, co), bias=_at(bias, 0), scale_a=_at(scale_a, 0), scale_b=_at(scale_b, 0),
                            part=_at(part, 0), zeros=_at(z, 0), lda=lda, a_bstride=abs_, a_segstride=ass, ldb=ldb, b_bstride=bbs, b_segstride=bss, ldc=ldc,
                            cstride=cs, a_seglen=asl, b_seglen=bsl, M=M, N=N, K=K, batch=batch,
                            flags=(1 if ta else 0) | (2 if tb else 0) | (4 if accumulate else 0), row_period=row_mask[0], row_off=row_mask[1],
                            row_lo=row_mask[2], row_hi=row_mask[3], rm_T=rm[0], rm_TP=rm[1], ksplit=ksplit, cfg=cfg, bf16=1 if bf16 else 0)
    _capi.check(_capi.lib().ss_op_gemm_img_desc(C.byref(d), _stream()))
    return c
