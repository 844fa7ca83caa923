#!/usr/bin/env python3
"""Write tests/golden/vocab/spans_gpt2u.json and tests/golden/vocab/spans_cl100k.json: per rule the texts of the
committed vocabulary fixture (vocab_gpt2u.json / vocab_cl100k.json, read and left as they are) and the additional
ones below, with the ids and the character offsets (Encoding.offsets) that the Hugging Face `tokenizers` library
gives for them with add_special_tokens=False.  The tokenizer.json is the committed fixture's and is not stored
again.  tests/test_spans_host.py and tests/test_gpu_spans.py hold the char unit of the token spans to them.

CPU only; needs `tokenizers`; no GPU.  Before anything is written the recorded offsets are held against the char
rule of tests/spans_ref.py, and at least 50 recorded tokens per file must begin or end inside a character: without
those the rule is not exercised.

    python tools/make_spans_golden.py
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from llmtokenizer_amd.vocab import Vocab  # noqa: E402
import spans_ref as SR  # noqa: E402

MORE_TEXTS = [
    "é ñ ü ß ø and Ελληνικά",                                  # 2-byte characters
    "€ ₤ 한글 日本 ‰ → ✓",                                       # 3-byte characters
    "😀 😃 𝄞 🚀 𠮷野家 😀😀😀",                                    # 4-byte characters
    "👨‍👩‍👧‍👦 family, 🏳️‍🌈 flag and ❤️‍🔥 heart",                       # ZWJ sequences
    "e\u0301 a\u0308 n\u0303 o\u0302\u0323 combining marks",          # combining marks
    "line\r\n\r\nnext\r\n\r\n\r\nend\r\n",                      # CRLF runs
    "   leading spaces and trailing spaces   ",
    "<|endoftext|>a special at the start 😀",
    "a special <|im_start|> in the middle 👍🏽 of 日本語",
    "a special at the end 🚀<|endoftext|>",
    "",
    "👍🏽👍🏽 ½ ¾ ™ © ® µ ¿ ¡ § ¶ † ‡ • ‹ › « »",
    "mixed\r\n😀\r\n<|im_start|>\r\né\r\n",
]


def main():
    from tokenizers import Tokenizer
    out_dir = os.path.join(ROOT, "tests", "golden", "vocab")
    for src, name in (("vocab_gpt2u", "spans_gpt2u"), ("vocab_cl100k", "spans_cl100k")):
        with open(os.path.join(out_dir, src + ".json"), encoding="utf-8") as f:
            fx = json.load(f)
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "tokenizer.json")
            with open(p, "w", encoding="utf-8") as f:
                json.dump(fx["tokenizer_json"], f, ensure_ascii=False)
            tok = Tokenizer.from_file(p)
            vocab = Vocab.from_tokenizer_json(p)
        assert fx["tokenizer_json"].get("post_processor") is None
        token_of = SR.token_bytes_by_id(vocab)
        texts = list(fx["texts"]) + MORE_TEXTS
        ids, offsets, inside = [], [], 0
        for k, text in enumerate(texts):
            enc = tok.encode(text, add_special_tokens=False)
            if k < len(fx["texts"]):
                assert enc.ids == fx["ids"][k], text
            raw = text.encode("utf-8")
            toks = [token_of[i] for i in enc.ids]
            want = SR.spans_of_text(toks, raw, "char")
            assert [tuple(o) for o in enc.offsets] == want, f"{name}: the char rule and `tokenizers` disagree on {text!r}"
            for bs, be in SR.spans_of_text(toks, raw, "byte"):
                inside += (raw[bs] & 0xC0) == 0x80 or (be < len(raw) and (raw[be] & 0xC0) == 0x80)
            ids.append(enc.ids)
            offsets.append([list(o) for o in enc.offsets])
        assert inside >= 50, f"{name}: only {inside} tokens begin or end inside a character"
        path = os.path.join(out_dir, name + ".json")
        with open(path, "w", encoding="utf-8") as f:
            json.dump({"rule": fx["rule"], "vocab": src, "texts": texts, "ids": ids, "offsets": offsets}, f,
                      ensure_ascii=False, separators=(",", ":"))
        print(f"{path}: {len(texts)} texts, {sum(map(len, ids))} tokens, {inside} of them begin or end inside a "
              f"character, {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 100_000


if __name__ == "__main__":
    main()
