#!/usr/bin/env python3
"""Write a decoding-graph image (m3asr.wfst.DecodingGraph, *.npy) from a lexicon file: the CTC token topology composed with the
lexicon as a free word loop, for decoding with a closed vocabulary and unigram word scores without OpenFst.

  python tools/make_lexicon_graph.py lexicon.txt --vocab-size V -o graph.npy [--units units.txt] [--words-out words.txt]
                                     [--word-costs costs.txt] [--blank 0]

lexicon.txt: `word tok tok ...` per line; a word on several lines has several pronunciations.  Tokens are token ids, or symbols
of units.txt (`token id` per line).  Word ids are given in order of first appearance, from 1; --words-out writes them as
`word id` lines (what infer.py --words reads).  costs.txt: `word cost` per line (default 0.0 each; a cost is -log probability).
The image is validated by the library before it is written."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3m-asr-inference_amd"))

from m3asr.wfst import DecodingGraph, read_lexicon


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lexicon")
    ap.add_argument("--vocab-size", type=int, required=True)
    ap.add_argument("-o", "--out", required=True)
    ap.add_argument("--units")
    ap.add_argument("--words-out")
    ap.add_argument("--word-costs")
    ap.add_argument("--blank", type=int, default=0)
    args = ap.parse_args()
    try:
        lexicon, words = read_lexicon(args.lexicon, args.units)
        costs = None
        if args.word_costs:
            ids = {w: i + 1 for i, w in enumerate(words)}
            costs = {}
            with open(args.word_costs, encoding="utf-8") as f:
                for line in f:
                    parts = line.split()
                    if parts:
                        costs[ids[parts[0]]] = float(parts[1])
        graph = DecodingGraph.from_lexicon(lexicon, args.vocab_size, args.blank, costs).validate()
    except (ValueError, KeyError, OSError) as e:
        raise SystemExit("make_lexicon_graph: %s" % e)
    graph.save(args.out)
    if args.words_out:
        with open(args.words_out, "w", encoding="utf-8") as f:
            f.write("<eps> 0\n" + "".join("%s %d\n" % (w, i + 1) for i, w in enumerate(words)))
    print("%s: %d words, %d states, %d arcs, %d levels, %d bytes" % (args.out, len(words), graph.n_states, graph.n_arcs,
                                                                     graph.n_levels, graph.image.nbytes))


if __name__ == "__main__":
    main()
