#!/usr/bin/env python3
"""Write tests/golden/vocab/vocab_nfc.json: texts that NFC changes and the ids the Hugging Face `tokenizers` library
gives for them under the vocabulary of tests/golden/vocab/vocab_cl100k.json written with "normalizer": {"type":
"NFC"} (Vocab.to_tokenizer_json), add_special_tokens=False.  tests/test_gpu_vocab_normalize.py holds the device to
them.  The fixture holds the texts and ids alone; the vocabulary is vocab_cl100k.json's.

CPU only; needs `tokenizers` and the built library.  Every text uses only code points Unicode 13 assigns, and before
anything is written `tokenizers`' normalizer is held against api.nfc_host on each, so that its newer tables and the
committed ones agree on the fixture.

    python tools/make_vocab_nfc_golden.py
"""
import json
import os
import sys
import tempfile
import unicodedata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from llmtokenizer_amd import api  # noqa: E402
from llmtokenizer_amd.vocab import Vocab  # noqa: E402

TEXTS = [
    '',
    'plain text that NFC leaves alone, 12345',
    'cafe\u0301 and cafe\u0301s, nai\u0308ve',
    'a\u0301\u0323 marks out of order, a\u0323\u0301 in order',
    '\u1100\u1161\u11a8 \uac00\u11a8 Hangul jamo',
    '\u0958\u0959 Devanagari exclusions \u0915\u093c',
    '\u212b ngstr\xf6m, \u2126 ohm, \xc5',
    'Gr\xf6\xdfe o\u0308 U\u0308bung<|endoftext|>\u0301 after a special',
    'a\u0327\u0327\u0301 blocked, \u1e0b\u0323 twice',
    '\u3099 alone, \u304b\u3099 ga',
]


def main():
    from tokenizers import Tokenizer
    out_dir = os.path.join(ROOT, "tests", "golden", "vocab")
    with open(os.path.join(out_dir, "vocab_cl100k.json"), encoding="utf-8") as f:
        base = json.load(f)
    with tempfile.TemporaryDirectory() as d:
        tmp = os.path.join(d, "tokenizer.json")
        with open(tmp, "w", encoding="utf-8") as f:
            json.dump(base["tokenizer_json"], f, ensure_ascii=False)
        plain = Vocab.from_tokenizer_json(tmp)
        vocab = Vocab(plain.merges, plain.byte_ids, plain.merge_ids, plain.special_ids, plain.specials, plain.rule, normalizer="nfc")
        vocab.to_tokenizer_json(tmp)
        assert Vocab.from_tokenizer_json(tmp, normalizers=("NFC",)) == vocab
        tok = Tokenizer.from_file(tmp)
    ids = []
    for text in TEXTS:
        assert all(unicodedata.category(c) != "Cn" for c in text), text  # (assigned in this Python's Unicode 13)
        norm = tok.normalizer.normalize_str(text)
        assert norm.encode() == api.nfc_host(text.encode()), f"`tokenizers` and nfc_host disagree on {text!r}"
        ids.append(tok.encode(text, add_special_tokens=False).ids)
    path = os.path.join(out_dir, "vocab_nfc.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"base": "vocab_cl100k.json", "normalizer": "nfc", "texts": TEXTS, "ids": ids}, f, ensure_ascii=True,
                  separators=(",", ":"))
    print(f"{path}: {len(TEXTS)} texts, {sum(map(len, ids))} ids, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
