#!/usr/bin/env python3
"""Run an encoder plan -- same command line as the reference's infer.py (:130-137):

    python3 infer.py -p encoder.plan -i feat.npy [-o compare.npy]
    python3 infer.py -p encoder.plan -w speech.wav [-o compare.npy]

feat.npy is (B,T,idim) float32; feat_len = feat.shape[1] for every utterance, as in the reference (infer.py:111-113).
speech.wav (-w, instead of -i) is a 16 kHz mono 16-bit RIFF file; its log-Mel frames are computed on the device by the
library's Kaldi-style front end (m3asr.frontend.Fbank with the plan's input_dim mel bins) and run as a batch of one.
Prints ``time=...ms`` for one forward after a warm-up and the output's shape / sum (reference :81-103)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "3m-asr-inference_amd"))

import numpy as np

import trt_helper
from trt_helper import trt


def read_wav(path):
    """16 kHz mono 16-bit PCM -> (1, N) int16"""
    import wave
    with wave.open(path, "rb") as w:
        if (w.getframerate(), w.getnchannels(), w.getsampwidth()) != (16000, 1, 2):
            raise SystemExit("%s: need 16 kHz mono 16-bit PCM, got %d Hz, %d channel(s), %d-bit" % (
                path, w.getframerate(), w.getnchannels(), 8 * w.getsampwidth()))
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.int16).reshape(1, -1)


def main(args):
    logger = trt_helper.init_trt_plugin(trt.Logger.INFO, "libm3asr_hip.so")
    helper = trt_helper.InferHelper(args.plan_name, logger)
    if args.wav_file:
        from m3asr.frontend import Fbank
        feat = Fbank(helper.cfg.input_dim, helper.engine.device)(read_wav(args.wav_file))[0].cpu().numpy()
    else:
        feat = np.load(args.input_file).astype(np.float32)
    feat_len = np.full((1, feat.shape[0]), feat.shape[1], dtype=np.int32)
    base = [np.load(args.compare_output_file)] if args.compare_output_file else None
    outputs = helper.infer([feat, feat_len], base)
    for o in outputs:
        print("outputs.shape:" + str(o.shape))
        print("outputs.sum:" + str(o.sum()))
        print(o)
    if base is not None:
        print("compare_output=%s, dtype=%s, shape=%s" % (args.compare_output_file, base[0].dtype, base[0].shape))
        print("output.sum:" + str(base[0].sum()))


if __name__ == "__main__":
    p = argparse.ArgumentParser(description="3M-ASR encoder inference (MI355X)")
    p.add_argument("-p", "--plan_name", required=True, help="The plan file path.")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("-i", "--input_file", help="The input feat.npy file path.")
    src.add_argument("-w", "--wav", dest="wav_file", help="A 16 kHz mono 16-bit wav file, instead of feat.npy.")
    p.add_argument("-o", "--compare_output_file", required=False, help="The compare output .npy file path.")
    main(p.parse_args())
