"""CTC forced alignment on the device: when each token of a hypothesis was spoken (include/m3asr.h, m3_ctc_align_*).

    aligner = CtcAligner(V)
    for a in aligner.align(logits, lens, [[5, 9, 9], [7]]):     # logits (B, T, V) on the device
        if a.ok:
            print(list(zip(a.tokens, a.start_ms, a.end_ms, a.conf)))

The token sequences may come from any decoding mode: the aligner needs the CTC logits and the tokens, nothing about how they
were found.  Two launches per call (emissions, then trellis + backtrace + spans), one copy back.  There is no CPU fallback.
"""
import collections

import torch

from . import ops

# One utterance's alignment.  tokens: the tokens asked for; start / end / peak: per token its first frame, the frame behind its
# last one and the frame of its largest posterior; conf: that posterior; score: the log-probability of the best alignment;
# states: the trellis state of every frame (even: the blank between tokens s / 2 - 1 and s / 2, odd: token s // 2);
# ok: an alignment exists (otherwise the per-token lists are empty, states is empty and score is -inf);
# start_ms / end_ms / peak_ms: the frame indices times the aligner's frame_ms.
Alignment = collections.namedtuple("Alignment", "tokens start end peak conf score states ok start_ms end_ms peak_ms")


class CtcAligner:
    """aligner = CtcAligner(V, blank=0, device="cuda", frame_ms=40); frame_ms: the encoder's output frame shift."""

    def __init__(self, V, blank=0, device="cuda", frame_ms=40):
        self.V, self.blank, self.frame_ms = int(V), int(blank), frame_ms
        self.device = torch.device(device)
        ops.ctc_align_desc(1, self.V, self.blank, 1, 1)          # refuses a bad (V, blank) now, not at the first call
        self.workspace = None                                     # the move table: grows with the batches, never shrinks

    def _check_tokens(self, tokens):
        out = []
        for u, y in enumerate(tokens):
            y = [int(v) for v in y]
            for v in y:
                if v == self.blank or not 0 <= v < self.V:
                    raise ValueError("CtcAligner: utterance %d holds token %d (blank = %d, V = %d)" % (u, v, self.blank, self.V))
            out.append(y)
        return out

    def align(self, logits, lens, tokens):
        """logits (B, T, V) f32 on the device, lens (B,) frames of each utterance that count, tokens: one token list per
        utterance -> [Alignment] * B."""
        B, T, V = logits.shape
        rows = logits.reshape(B * T, V)
        n_frames = [int(v) for v in torch.as_tensor(lens).reshape(-1).tolist()]
        if len(n_frames) != B or any(not 0 <= v <= T for v in n_frames):
            raise ValueError("CtcAligner.align: lens %s for a batch of %d x %d frames" % (n_frames, B, T))
        return self.align_rows(rows, [b * T for b in range(B)], n_frames, tokens)

    def align_rows(self, rows, row0, n_frames, tokens):
        """Packed, ragged utterances: rows (R, ld) f32 on the device (a row-strided view with V columns is fine), utterance u
        = rows row0[u] .. row0[u] + n_frames[u]; row0 / n_frames: lists or int32 tensors -> [Alignment] per utterance."""
        tokens = self._check_tokens(tokens)             # before anything is launched
        n = len(tokens)
        row0 = torch.as_tensor(row0).reshape(-1).to(torch.int32)
        n_frames = torch.as_tensor(n_frames).reshape(-1).to(torch.int32)
        if row0.numel() != n or n_frames.numel() != n:
            raise ValueError("CtcAligner: %d token lists, %d row0, %d n_frames" % (n, row0.numel(), n_frames.numel()))
        if n == 0:
            return []
        if rows.dim() != 2 or rows.shape[1] != self.V:
            raise ValueError("CtcAligner: rows of shape %s, need (R, %d)" % (tuple(rows.shape), self.V))
        frames = n_frames.cpu().tolist()
        first = row0.cpu().tolist()
        if any(f < 0 or r < 0 or r + f > rows.shape[0] for r, f in zip(first, frames)):
            raise ValueError("CtcAligner: an utterance's rows lie outside the %d rows given" % rows.shape[0])
        desc = ops.ctc_align_desc(n, self.V, self.blank, max(frames), max(len(y) for y in tokens))
        need = ops.ctc_align_workspace_size(desc)
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        tok0 = [0]
        for y in tokens:
            tok0.append(tok0[-1] + len(y))
        dev = self.device
        # one upload: row0 | n_frames | tok0 | tokens
        host = torch.tensor(first + frames + tok0 + [v for y in tokens for v in y], dtype=torch.int32)
        meta = host.to(dev)
        d_row0, d_frames, d_tok0, d_tokens = meta[:n], meta[n:2 * n], meta[2 * n:3 * n + 1], meta[3 * n + 1:]
        emit = ops.ctc_align_emit(desc, rows, d_row0, d_frames, d_tokens, d_tok0)
        # one buffer for the seven outputs (4-byte elements all), so that one copy brings them back
        sizes = [n, n, n * desc.max_frames] + [tok0[-1]] * 4
        res = torch.empty(sum(sizes), dtype=torch.int32, device=dev)
        f32 = lambda t: t.view(torch.float32)
        part = res.split(sizes)
        ops.ctc_align_path(desc, emit, d_frames, d_tokens, d_tok0, self.workspace,
                           out=(f32(part[0]), part[1], part[2].view(n, desc.max_frames), part[3], part[4], part[5], f32(part[6])))
        part = res.cpu().split(sizes)
        score, status, state = f32(part[0]).tolist(), part[1].tolist(), part[2].view(n, desc.max_frames)
        ts, te, tp, conf = part[3].tolist(), part[4].tolist(), part[5].tolist(), f32(part[6]).exp().tolist()
        out = []
        ms = self.frame_ms
        for u, y in enumerate(tokens):
            if status[u] != 0:
                out.append(Alignment(y, [], [], [], [], float("-inf"), [], False, [], [], []))
                continue
            lo, hi = tok0[u], tok0[u + 1]
            out.append(Alignment(y, ts[lo:hi], te[lo:hi], tp[lo:hi], conf[lo:hi], score[u], state[u, :frames[u]].tolist(), True,
                                 [t * ms for t in ts[lo:hi]], [t * ms for t in te[lo:hi]], [t * ms for t in tp[lo:hi]]))
        return out


def token_times(a, frame_ms, offset_frames=0):
    """[(token, start_ms, end_ms, conf)] of an Alignment whose frame 0 is frame offset_frames of something longer (a segment
    in its session): (offset_frames + frame) * frame_ms.  None for an utterance that has no alignment."""
    if a is None or not a.ok:
        return None
    return [(tok, (offset_frames + s) * frame_ms, (offset_frames + e) * frame_ms, c)
            for tok, s, e, c in zip(a.tokens, a.start, a.end, a.conf)]
