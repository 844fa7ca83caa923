"""Vocabulary files on the host (llmtokenizer_amd/vocab.py, src/bpe_vocab.c); no GPU.  Both loaders run
on vocabularies written here (a few hundred merges trained by tests/train_split_ref.py, shuffled ids
with holes, two specials); every refusal names its cause; bpe_vocab_check and bpe_vocab_tables are held
to restatements; and where `tokenizers` imports, its ids for the exported file equal a Python
rank-order replay mapped through the Vocab."""
import base64
import copy
import json

import numpy as np
import pytest

import train_split_ref as R
from llmtokenizer_amd import api
from llmtokenizer_amd.api import BpeError
from llmtokenizer_amd.synth import english_like
from llmtokenizer_amd.vocab import CL100K_PATTERN, Vocab, replay, vocab_tables

SPECIALS = [b"<|endoftext|>", b"<|pad|>"]
RULES = ["gpt2_unicode", "cl100k"]
EXTRA = " It's 2024, we've 1234567 things; they'll say: naïve café, Größe, 日本語!\n\n\tdone\r\n"


def corpus():
    return english_like(5000) + (EXTRA * 8).encode()


def pieces_of(data, rule, specials=None):
    off = api.split_host(data, rule, specials).tolist()
    return [data[a:b] for a, b in zip(off, off[1:])]


def make_vocab(rule, seed=5, n_merges=250):
    merges, _, _ = R.train(pieces_of(corpus(), rule), n_merges)
    assert len(merges) == n_merges
    ids = np.random.default_rng(seed).permutation(256 + n_merges + 40)[: 256 + n_merges]
    return Vocab(merges, ids[:256], ids[256:], [70000, 9_000_000], SPECIALS, rule)


@pytest.fixture(scope="module", params=RULES)
def voc(request):
    return make_vocab(request.param)


@pytest.fixture(scope="module")
def doc(tmp_path_factory):
    """the tokenizer.json of a gpt2_unicode vocabulary, as an object the refusal tests edit"""
    p = tmp_path_factory.mktemp("vocab") / "tokenizer.json"
    make_vocab("gpt2_unicode", n_merges=60).to_tokenizer_json(p)
    return json.loads(p.read_text(encoding="utf-8"))


def load_doc(d, tmp_path):
    p = tmp_path / "t.json"
    p.write_text(json.dumps(d, ensure_ascii=False), encoding="utf-8")
    return Vocab.from_tokenizer_json(p)


def host_ids(v, data):
    """rank-order replay inside the pieces, mapped through the vocabulary"""
    rank = {tuple(p): r for r, p in enumerate(v.merges.tolist())}
    sp = {s: int(i) for s, i in zip(v.specials, v.special_ids)}
    fwd = np.concatenate([v.byte_ids, v.merge_ids])
    out = []
    for p in pieces_of(data, v.rule, v.specials):
        out += [sp[p]] if p in sp else [int(fwd[i]) for i in replay(list(p), rank)]
    return out


# ---------------------------------------------------------------- the loaders

def test_tokenizer_json_round_trip(voc, tmp_path):
    p = tmp_path / "tokenizer.json"
    voc.to_tokenizer_json(p)
    back = Vocab.from_tokenizer_json(p)
    assert back == voc
    assert back.rule == voc.rule and back.specials == SPECIALS and back.special_ids.tolist() == [70000, 9_000_000]


def test_merges_are_read_in_both_spellings(voc, tmp_path):
    p = tmp_path / "tokenizer.json"
    voc.to_tokenizer_json(p)
    d = json.loads(p.read_text(encoding="utf-8"))
    assert all(isinstance(m, str) for m in d["model"]["merges"])
    d["model"]["merges"] = [m.split(" ") for m in d["model"]["merges"]]
    assert load_doc(d, tmp_path) == voc


def test_ignore_merges_is_accepted(doc, tmp_path):
    d = copy.deepcopy(doc)
    d["model"]["ignore_merges"] = True
    assert load_doc(d, tmp_path) == load_doc(doc, tmp_path)


def monotone(v):
    """v with merge ids that grow with the rank, as a rank file needs them (its rank is the id and the priority);
    the byte ids stay shuffled"""
    ids = np.sort(np.random.default_rng(9).permutation(5000)[: 256 + v.merges.shape[0]])
    return Vocab(v.merges, np.random.default_rng(1).permutation(ids[:256]), ids[256:], [6000, 6001], SPECIALS, v.rule)


def test_rank_file_gives_the_same_merges(voc, tmp_path):
    mono = monotone(voc)
    p = tmp_path / "ranks.tiktoken"
    mono.to_tiktoken(p)
    back = Vocab.from_tiktoken(p, voc.rule, dict(zip(SPECIALS, [6000, 6001])))
    assert back.merges.tolist() == voc.merges.tolist()
    assert back == mono


def test_rank_file_needs_ids_in_rank_order(voc, tmp_path):
    with pytest.raises(BpeError, match="grow with the rank"):
        voc.to_tiktoken(tmp_path / "ranks.tiktoken")


def test_identity_numbering():
    m = make_vocab("cl100k", n_merges=30).merges
    v = Vocab.from_merges(m, "cl100k", SPECIALS)
    fwd, inv = vocab_tables(v)
    assert fwd.tolist() == list(range(256 + 30 + 2)) and inv.tolist() == fwd.tolist()


def test_rank_file_with_a_token_no_merge_reaches(tmp_path):
    v = monotone(make_vocab("cl100k", n_merges=20))
    p = tmp_path / "ranks.tiktoken"
    v.to_tiktoken(p)
    with open(p, "ab") as f:
        f.write(base64.b64encode(b"qzqzq") + b" 5500\n")
    with pytest.raises(BpeError, match=r"1 token\(s\) cannot be reached.*qzqzq"):
        Vocab.from_tiktoken(p, "cl100k")


# ---------------------------------------------------------------- refusals of from_tokenizer_json

def _set(path, value):
    def edit(d):
        x = d
        for k in path[:-1]:
            x = x[k]
        x[path[-1]] = value
    return edit


REFUSALS = [
    ("add_prefix_space", _set(("pre_tokenizer", "add_prefix_space"), True), "add_prefix_space"),
    ("normalizer", _set(("normalizer",), {"type": "NFC"}), "normalizer"),
    ("byte_fallback", _set(("model", "byte_fallback"), True), "byte_fallback"),
    ("dropout", _set(("model", "dropout"), 0.1), "dropout"),
    ("prefix", _set(("model", "continuing_subword_prefix"), "##"), "continuing_subword_prefix"),
    ("suffix", _set(("model", "end_of_word_suffix"), "</w>"), "end_of_word_suffix"),
    ("lstrip", _set(("added_tokens", 0, "lstrip"), True), "lstrip"),
    ("rstrip", _set(("added_tokens", 1, "rstrip"), True), "rstrip"),
    ("single_word", _set(("added_tokens", 0, "single_word"), True), "single_word"),
    ("normalized", _set(("added_tokens", 1, "normalized"), True), "normalized"),
    ("whitespace", _set(("pre_tokenizer",), {"type": "Whitespace"}), "Whitespace"),
    ("no_regex", _set(("pre_tokenizer", "use_regex"), False), "use_regex"),
    ("model_type", _set(("model", "type"), "WordPiece"), "WordPiece"),
    ("o200k", _set(("pre_tokenizer",), {"type": "Sequence", "pretokenizers": [
        {"type": "Split", "pattern": {"Regex": r"[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}]*[\p{Ll}]+|\p{N}{1,3}"},
         "behavior": "Isolated", "invert": False},
        {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": False}]}), r"\\p\{Lu\}"),
    ("removed", _set(("pre_tokenizer",), {"type": "Sequence", "pretokenizers": [
        {"type": "Split", "pattern": {"Regex": CL100K_PATTERN}, "behavior": "Removed", "invert": False},
        {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": False}]}), "Removed"),
]


@pytest.mark.parametrize("name,edit,names", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_their_cause(doc, tmp_path, name, edit, names):
    d = copy.deepcopy(doc)
    edit(d)
    with pytest.raises(BpeError, match=names):
        load_doc(d, tmp_path)


def test_the_cl100k_sequence_is_accepted(doc, tmp_path):
    d = copy.deepcopy(doc)
    d["pre_tokenizer"] = {"type": "Sequence", "pretokenizers": [
        {"type": "Split", "pattern": {"Regex": CL100K_PATTERN}, "behavior": "Isolated", "invert": False},
        {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": False}]}
    assert load_doc(d, tmp_path).rule == "cl100k"


def test_an_unreachable_token_is_named(doc, tmp_path):
    d = copy.deepcopy(doc)
    d["model"]["vocab"]["zzqzz"] = 4242
    with pytest.raises(BpeError, match=r"1 token\(s\) cannot be reached.*zzqzz.*4242"):
        load_doc(d, tmp_path)


def test_a_token_the_merges_reach_another_way_is_named(doc, tmp_path):
    """a merge whose result an earlier, lower-rank merge pre-empts: its bytes do not replay to its id"""
    d = copy.deepcopy(doc)
    a, b = d["model"]["merges"][0].split(" ")
    c = next(ch for ch in "qxzjk" if a + b + ch not in d["model"]["vocab"])
    # (b + c) after (a + b): in the text a b c the first merge wins, so the token a + (b c) is unreachable
    d["model"]["vocab"][b + c] = 5001
    d["model"]["vocab"][a + b + c] = 5002
    d["model"]["merges"] += [f"{b} {c}", f"{a} {b + c}"]
    with pytest.raises(BpeError, match=r"cannot be reached.*5002"):
        load_doc(d, tmp_path)


def test_a_missing_byte_and_a_dangling_merge_are_named(doc, tmp_path):
    d = copy.deepcopy(doc)
    del d["model"]["vocab"]["!"]
    with pytest.raises(BpeError, match="byte 0x21"):
        load_doc(d, tmp_path)
    d = copy.deepcopy(doc)
    d["model"]["merges"].insert(0, "qq zz")
    with pytest.raises(BpeError, match="merge 0"):
        load_doc(d, tmp_path)


# ---------------------------------------------------------------- bpe_vocab_check / bpe_vocab_tables

def test_check_refuses_duplicates_large_ids_and_later_parts():
    v = make_vocab("cl100k", n_merges=20)
    args = dict(merges=v.merges, byte_ids=v.byte_ids, merge_ids=v.merge_ids, special_ids=v.special_ids,
                specials=SPECIALS, rule="cl100k")

    def refused(match, **kw):
        a = {k: np.array(x) if isinstance(x, np.ndarray) else x for k, x in {**args, **kw}.items()}
        with pytest.raises(BpeError, match=match):
            Vocab(**a)

    dup = v.merge_ids.copy()
    dup[7] = v.byte_ids[0x41]
    refused("byte 0x41 and merge 7 share the id", merge_ids=dup)
    refused("special 0 and special 1 share", special_ids=[70000, 70000])
    refused(r"special 1 has the id 16777216, at or above 2\^24", special_ids=[70000, 1 << 24])
    Vocab(**{**args, "special_ids": [70000, (1 << 24) - 1]})  # the largest id allowed
    late = v.merges.copy()
    late[3, 1] = 256 + 3
    refused("merge 3 names the id 259 as its second part", merges=late)
    refused("numbers 19 merges, the merge list holds 20", merge_ids=v.merge_ids[:19])
    with pytest.raises(BpeError, match="one id per special"):
        Vocab(**{**args, "special_ids": [70000]})


def test_tables_equal_a_numpy_restatement(voc):
    fwd, inv = vocab_tables(voc)
    want = np.concatenate([voc.byte_ids, voc.merge_ids, voc.special_ids])
    assert fwd.dtype == np.uint32 and fwd.tolist() == want.tolist()
    winv = np.full(int(want.max()) + 1, 0xFFFFFFFF, dtype=np.uint32)
    winv[want] = np.arange(want.size, dtype=np.uint32)
    assert inv.size == voc.size == winv.size and (inv == winv).all()
    assert int((inv == 0xFFFFFFFF).sum()) == inv.size - want.size > 0


# ---------------------------------------------------------------- the outside oracle

def random_texts(count, seed):
    rng = np.random.default_rng(seed)
    bits = ["the", "The", " of", "ing", "and", " ", "  ", "\n", "\n\n", "\t", "'s", "'ll", "'RE", "don't", "1", "23", "4567",
            "89012", ".", ",", "!?", "...", "é", "ü", "ß", "日本", "語", "я", "Ж", "€", "—", "<|endoftext|>", "<|pad|>", "<|", "|>",
            "x", "q", "zz", "e", "t", "a", "o", "\r\n", " \n", "_", "(", ")"]
    return ["".join(bits[i] for i in rng.integers(0, len(bits), int(rng.integers(0, 40)))) for _ in range(count)]


def test_tokenizers_gives_the_ids_of_the_host_replay(voc, tmp_path):
    tokenizers = pytest.importorskip("tokenizers")
    p = tmp_path / "tokenizer.json"
    voc.to_tokenizer_json(p)
    tok = tokenizers.Tokenizer.from_file(str(p))
    texts = random_texts(300, 17)
    assert sum("<|endoftext|>" in t for t in texts) > 20
    for t in texts:
        assert tok.encode(t, add_special_tokens=False).ids == host_ids(voc, t.encode("utf-8")), repr(t)


# ---------------------------------------------------------------- the kernels' resources

def test_map_kernels_have_no_scratch_and_no_lds():
    """k_ids_map and k_ids_unmap stream ids: no private segment, no LDS (read from the gfx950 kernel
    descriptors of the built library, as tests/test_abi.py does for the per-merge kernels)"""
    import importlib.util
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_scratch", os.path.join(root, "tools", "kernel_scratch.py"))
    ks = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ks)
    kd = ks.scan(os.environ.get("BPE_LIB") or os.path.join(root, "llmtokenizer_amd", "libbpe_amd.so"))
    found = {k: v for k in ("k_ids_map", "k_ids_unmap") for name, v in kd.items() if re.search(r"\d%sE" % k, name)}
    assert set(found) == {"k_ids_map", "k_ids_unmap"}, sorted(found)
    assert all(v == (0, 0) for v in found.values()), found
