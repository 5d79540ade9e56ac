"""Host side of streaming two-pass decoding: the shapes a service sees, and the ABI table.  No device."""
import inspect


def test_segment_shapes():
    from m3asr.serve import RescoredSegment, Segment
    assert Segment._fields == ("rule", "start_ms", "end_ms", "nbest", "end_frame")       # unchanged: callers compare tuple(segment)
    assert RescoredSegment._fields == Segment._fields + ("best", "scores")
    seg = Segment(1, 0, 400, [((3, 4), -1.5)], 9)
    two = RescoredSegment(*seg, (3, 4), [((3, 4), -1.5, -2.0, -2.75)])
    assert tuple(two)[:5] == tuple(seg) and two.best == (3, 4) and two.scores[0][3] == -2.75


def test_public_signatures():
    from m3asr.decode import StreamingCtcDecoder
    from m3asr.rescore import AttentionRescorer
    from m3asr.serve import StreamPool
    p = inspect.signature(StreamingCtcDecoder.__init__).parameters
    assert (p["rescorer"].default, p["ctc_weight"].default, p["reverse_weight"].default) == (None, 0.5, 0.0)
    p = inspect.signature(StreamingCtcDecoder.rescore).parameters
    assert (p["slots"].default, p["detail"].default) == (None, False)
    assert inspect.signature(StreamPool.__init__).parameters["rescore"].default is False
    assert inspect.signature(StreamPool.close).parameters["rescored"].default is False
    assert inspect.signature(AttentionRescorer.rescore_rows).parameters["raw_memory"].default is True


def test_memory_entry_points_are_in_the_abi_table():
    import ctypes
    from m3asr import _lib
    names = ["m3_aed_memory_state_size", "m3_aed_memory_reset", "m3_aed_memory_reset_slots", "m3_aed_memory_append",
             "m3_aed_memory_lengths", "m3_aed_memory_gather"]
    assert all(n in _lib.SIGNATURES for n in names)
    assert ctypes.sizeof(_lib.AedMemoryDesc) == 12
    # the size query is pure host arithmetic: a header and max_frames rows of D floats per slot, whole 256 bytes
    lib = _lib.load()
    size = lambda B, T, D: lib.m3_aed_memory_state_size(ctypes.byref(_lib.AedMemoryDesc(B, T, D)))   # noqa: E731
    assert size(3, 12, 32) == 3 * (256 + 12 * 32 * 4) and size(1, 5, 4) == 512 and size(0, 12, 32) == 0
    assert size(3, 12, 30) == 0 and b"multiple of 4" in lib.m3_last_error()
    assert size(3, -1, 32) == 0 and size(-1, 12, 32) == 0
