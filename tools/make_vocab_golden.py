#!/usr/bin/env python3
"""Write tests/golden/vocab/vocab_gpt2u.json and tests/golden/vocab/vocab_cl100k.json (a directory of their own:
tests/golden_lib.py reads every *.json directly under tests/golden as a training fixture): per rule a synthetic
tokenizer.json (a few hundred merges trained by tests/train_split_ref.py on the text below, shuffled ids
with holes, specials with far-away ids), some thirty texts and the ids the Hugging Face `tokenizers`
library gives for them (add_special_tokens=False).  tests/test_gpu_vocab.py holds the device to them.

CPU only; needs `tokenizers` and the built library (for split_host, no GPU).  Before anything is written
the pieces of api.split_host are held against the pre-tokenizer's for every text, segment by segment
between the specials: a disagreement (a character whose class the committed Unicode table and the one
inside `tokenizers` see differently, say) fails the run instead of hiding in the fixture.

    python tools/make_vocab_golden.py
"""
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from llmtokenizer_amd import api  # noqa: E402
from llmtokenizer_amd.vocab import CHAR_TO_BYTE, Vocab, replay  # noqa: E402
import train_split_ref as R  # noqa: E402

MERGES = 300
SPECIALS = ["<|endoftext|>", "<|im_start|>"]
SPECIAL_IDS = {"gpt2_unicode": [50256, 100264], "cl100k": [100257, 128000]}

CORPUS = """\
The quick brown fox jumps over the lazy dog. The dog didn't mind; it's what foxes do, isn't it?
We've seen 12 foxes, 345 dogs and 6789 birds since 2019, and they're all over the hills.
I'll say it again: the numbers 1000000 and 31415926 don't mean much.  She'd said so, he'd agreed.
Größe, Straße, Übung: die Füchse springen über den faulen Hund.  Ça va très bien, merci à vous.
Быстрая коричневая лиса прыгает через ленивую собаку, а собака спит.
日本語のテキストも少しだけ入れておきます。狐は犬を飛び越える。
def tokenize(text):\n    return [t for t in text.split() if t]\n\n\nprint(tokenize("a b  c"))\n
    x = y + 42;  // comment\n\ty -= 7;\r\n\r\nif (x != y) { return x * 100; }
Tabs\tand   spaces   and trailing blanks   \n\n\n   and newlines in runs.\n
"""

TEXTS = [
    "",
    "a",
    "Hello, world!",
    "The quick brown fox jumps over the lazy dog.",
    "I'll go; you're late, we've eaten, she'd know, I'm sure it's Tom's, don't!",
    "I'LL GO; YOU'RE LATE, WE'VE EATEN 'S 'T",
    "numbers: 1 22 333 4444 55555 666666 7777777 1234567890123",
    "3.14159 and 2,718,281 and 0x1F and 1e10 and 007",
    "line one\nline two\n\nline four\n\n\n\nline eight",
    "trailing spaces   \n   leading spaces\n\t\ttabs\r\nand crlf\r\n\r\n",
    "   ",
    "\n\n\n",
    " \n \n ",
    "Größe und Straße: die Übung für Füchse",
    "Ça va très bien, merci à vous, señor Nuñez",
    "Быстрая коричневая лиса прыгает через ленивую собаку",
    "日本語のテキスト。狐は犬を飛び越える123回。",
    "mixed: naïve café 42€ — “quoted” … ok",
    "digits next to letters: abc123def456 7days 2nd x86_64",
    "punctuation runs!!! ??? ... ;;; (((nested))) [brackets] {braces}\n\n",
    "x = y + 42;  // comment\n\ty -= 7;\n",
    "<|endoftext|>",
    "<|endoftext|><|im_start|><|endoftext|>",
    "Hello<|endoftext|>world",
    "spaces around <|endoftext|> a special and   <|im_start|>   more",
    "digits123<|endoftext|>456digits 789<|im_start|>0",
    "don't<|endoftext|>'t and it's<|im_start|>'s",
    "newlines\n\n<|endoftext|>\n\nafter\n<|im_start|>\n",
    "punct!!!<|endoftext|>??? ...<|im_start|>...",
    "Größe<|endoftext|>Übung 日本<|im_start|>語",
    "<|endoftext|> leading and trailing <|im_start|>",
    "almost special <|endoftext| > and <|im_start and |>",
]


def pieces_of(data, rule, specials=None):
    off = api.split_host(data, rule, specials).tolist()
    return [data[a:b] for a, b in zip(off, off[1:])]


def build_vocab(rule, seed):
    corpus = (CORPUS * 3 + " ".join(t for t in TEXTS if "<|" not in t)).encode("utf-8")
    merges, _, _ = R.train(pieces_of(corpus, rule), MERGES)
    k = len(merges)
    assert k >= 200, k
    rng = np.random.default_rng(seed)
    ids = rng.permutation(256 + k + 64)[: 256 + k]  # shuffled, with holes
    return Vocab(merges, ids[:256], ids[256:], SPECIAL_IDS[rule], [s.encode() for s in SPECIALS], rule)


def check_pieces(tok, vocab, text):
    """the pre-tokenizer's pieces, segment by segment between the specials, against split_host's"""
    want = []
    for seg in re.split("(" + "|".join(re.escape(s) for s in SPECIALS) + ")", text):
        if seg in SPECIALS:
            want.append(seg.encode())
        elif seg:
            want += [bytes(CHAR_TO_BYTE[c] for c in p) for p, _ in tok.pre_tokenizer.pre_tokenize_str(seg)]
    got = pieces_of(text.encode("utf-8"), vocab.rule, vocab.specials)
    assert got == want, f"{vocab.rule}: split_host and the pre-tokenizer disagree on {text!r}:\n{got}\n{want}"


def host_ids(vocab, text):
    """rank-order replay of the pieces, mapped through the vocabulary (what the device computes)"""
    rank = {tuple(p): r for r, p in enumerate(vocab.merges.tolist())}
    sp = {s: int(i) for s, i in zip(vocab.specials, vocab.special_ids)}
    fwd = np.concatenate([vocab.byte_ids, vocab.merge_ids])
    out = []
    for p in pieces_of(text.encode("utf-8"), vocab.rule, vocab.specials):
        out += [sp[p]] if p in sp else [int(fwd[i]) for i in replay(list(p), rank)]
    return out


def main():
    from tokenizers import Tokenizer
    out_dir = os.path.join(ROOT, "tests", "golden", "vocab")
    os.makedirs(out_dir, exist_ok=True)
    for rule, name, seed in (("gpt2_unicode", "vocab_gpt2u", 11), ("cl100k", "vocab_cl100k", 12)):
        vocab = build_vocab(rule, seed)
        tmp = os.path.join(out_dir, name + ".tokenizer.tmp")
        try:
            vocab.to_tokenizer_json(tmp)
            assert Vocab.from_tokenizer_json(tmp) == vocab
            tok = Tokenizer.from_file(tmp)
            with open(tmp, encoding="utf-8") as f:
                doc = json.load(f)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
        ids = []
        for text in TEXTS:
            assert "\0" not in text
            check_pieces(tok, vocab, text)
            got = tok.encode(text, add_special_tokens=False).ids
            assert got == host_ids(vocab, text), f"{rule}: `tokenizers` and the host replay disagree on {text!r}"
            ids.append(got)
        path = os.path.join(out_dir, name + ".json")
        with open(path, "w", encoding="utf-8") as f:
            json.dump({"rule": rule, "tokenizer_json": doc, "texts": TEXTS, "ids": ids}, f, ensure_ascii=False,
                      separators=(",", ":"))
        print(f"{path}: {len(vocab.merges)} merges, {len(TEXTS)} texts, {sum(map(len, ids))} ids, "
              f"{os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 200_000


if __name__ == "__main__":
    main()
