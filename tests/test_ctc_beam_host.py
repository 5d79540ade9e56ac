"""Host-side checks of the device CTC searches (no GPU): descriptor validation and state sizes of m3_ctc_beam_* /
m3_ctc_greedy_stream_*, and which decoding-chunk settings CtcDecoder accepts."""
import types

import pytest


def test_beam_desc_limits():
    from m3asr import ops
    from m3asr._lib import M3Error
    for beam, k in ((0, 1), (33, 4), (4, 0), (4, 33)):
        with pytest.raises(M3Error):
            ops.ctc_beam_desc(2, beam, 100, 0, k)
    with pytest.raises(M3Error):
        ops.ctc_beam_desc(2, 4, -1, 0)
    with pytest.raises(M3Error):
        ops.ctc_beam_desc(2, 4, 100, -1)
    d = ops.ctc_beam_desc(2, 32, 100, 0, 32)
    assert (d.B, d.beam, d.k, d.max_frames, d.blank) == (2, 32, 32, 100, 0)


def test_beam_state_size():
    from m3asr import ops
    one = ops.ctc_beam_state_size(ops.ctc_beam_desc(1, 10, 125, 0))
    # trie pool of 1 + frames x beam nodes (3 int32) and a hash table of >= 2x that many (int64 key + int32 node)
    assert one >= (1 + 125 * 10) * (12 + 2 * 12) and one % 256 == 0
    assert ops.ctc_beam_state_size(ops.ctc_beam_desc(16, 10, 125, 0)) == 16 * one
    assert ops.ctc_beam_state_size(ops.ctc_beam_desc(0, 10, 125, 0)) == 0
    assert ops.ctc_beam_state_size(ops.ctc_beam_desc(1, 10, 250, 0)) > one
    assert ops.ctc_beam_state_size(ops.ctc_beam_desc(1, 10, 0, 0)) > 0


def test_greedy_stream_desc_and_size():
    from m3asr import ops
    from m3asr._lib import M3Error
    d = ops.ctc_greedy_stream_desc(4, 200, 0)
    n = ops.ctc_greedy_stream_state_size(d)
    assert n >= 4 * 200 * 4 and n % 256 == 0
    with pytest.raises(M3Error):
        ops.ctc_greedy_stream_desc(4, -5, 0)


def test_decoder_chunk_settings():
    """decoding_chunk_size > 0 is accepted exactly when the engine was built with that static chunk mask."""
    from m3asr.config import EncoderConfig
    from m3asr.decode import CtcDecoder
    chunked = CtcDecoder(types.SimpleNamespace(cfg=EncoderConfig(static_chunk_size=16, num_decoding_left_chunks=2)))
    chunked._full_context(16, 2)
    chunked._full_context(-1, -1)
    for bad in ((8, 2), (16, -1), (16, 3)):
        with pytest.raises(NotImplementedError):
            chunked._full_context(*bad)
    full = CtcDecoder(types.SimpleNamespace(cfg=EncoderConfig()))
    with pytest.raises(NotImplementedError):
        full._full_context(16, -1)
    full._full_context(-1, -1)
