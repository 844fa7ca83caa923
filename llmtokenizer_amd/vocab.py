"""Vocabulary files: a tokenizer's own numbering over the engine's ids.

The engine numbers byte b as b, merge r as 256 + r and special j as 256 + merges + j.  A Vocab holds a
merge list, a preset split rule, the specials and the id each of those has in a vocabulary file; the
device rewrites ids between the two numberings (bpe_gpu.h, "Vocabularies": Engine.map_ids and the
vocab= keyword of Engine.decode_docs).  File formats are parsed here, in Python; C gets arrays.

Two loaders: Vocab.from_tokenizer_json (a byte-level BPE tokenizer.json of the Hugging Face
`tokenizers` library, GPT-2's or Llama 3's shape) and Vocab.from_tiktoken (a rank file).  Both refuse
what the engine does not reproduce, naming it, and both hold every token to reachability: a token is a
byte, a merge result or a special, and its own bytes replay to its single id.  Vocab.from_merges numbers
a list trained here the engine's own way, Vocab.to_tokenizer_json writes it for others to read.
"""
import base64
import ctypes
import json

import numpy as np

from . import _lib
from . import api
from ._lib import BpeError

# the cl100k_base / Llama 3 pre-tokenization pattern (bpe_gpu.h BPE_SPLIT_CL100K)
CL100K_PATTERN = (r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*"
                  r"|\s*[\r\n]+|\s+(?!\S)|\s+")
RULES = ("gpt2_unicode", "cl100k")  # the presets a vocabulary file can name
ID_LIMIT = 1 << 24


def _byte_alphabet():
    """GPT-2's byte-to-unicode alphabet: the printable Latin-1 bytes stand for themselves, the other 68
    are U+0100 onwards in byte order"""
    keep = list(range(0x21, 0x7F)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    chars, extra = {}, 0
    for b in range(256):
        if b in keep:
            chars[b] = chr(b)
        else:
            chars[b] = chr(256 + extra)
            extra += 1
    return chars


BYTE_TO_CHAR = _byte_alphabet()
CHAR_TO_BYTE = {c: b for b, c in BYTE_TO_CHAR.items()}


def _to_alphabet(raw):
    return "".join(BYTE_TO_CHAR[b] for b in raw)


def _from_alphabet(text, what):
    try:
        return bytes(CHAR_TO_BYTE[c] for c in text)
    except KeyError:
        raise BpeError(f"{what} {text!r} has a character outside the byte-level alphabet") from None


def replay(ids, rank):
    """ids (a list) with the merges of rank ({(a, b): r}, merge r makes the id 256 + r) applied lowest rank
    first, every occurrence from left to right: for a list whose merge r names only ids below 256 + r this is
    the rank-order replay of the encoders"""
    ids = list(ids)
    while len(ids) > 1:
        best = min((rank.get(p, ID_LIMIT) for p in zip(ids, ids[1:])))
        if best == ID_LIMIT:
            break
        out, i, z = [], 0, 256 + best
        while i < len(ids):
            if i + 1 < len(ids) and rank.get((ids[i], ids[i + 1])) == best:
                out.append(z)
                i += 2
            else:
                out.append(ids[i])
                i += 1
        ids = out
    return ids


class _CVocab:
    """bpe_gpu.h bpe_gpu_vocab over a Vocab's arrays (keeps the buffers it points to)"""

    def __init__(self, v):
        self.arrays = [np.ascontiguousarray(a, dtype=np.uint32) for a in (v.byte_ids, v.merge_ids, v.special_ids)]
        ptr = [a.ctypes.data if a.size else None for a in self.arrays]
        self.c = _lib.VocabIds(ptr[0], ptr[1], ptr[2], self.arrays[1].size, self.arrays[2].size)
        self.ref = ctypes.byref(self.c)


def vocab_tables(vocab):
    """(forward, inverse) tables of a Vocab as the device reads them (bpe_ex.h bpe_vocab_tables): forward maps
    internal id to vocabulary id, inverse the other way with 0xFFFFFFFF for a hole.  No GPU."""
    L = _lib.load()
    cv = vocab.c_vocab()
    nf, ni = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.check(L.bpe_vocab_tables(cv.ref, None, 0, None, 0, ctypes.byref(nf), ctypes.byref(ni)), "vocab_tables")
    fwd = np.zeros(nf.value, dtype=np.uint32)
    inv = np.zeros(ni.value, dtype=np.uint32)
    vp = ctypes.c_void_p
    _lib.check(L.bpe_vocab_tables(cv.ref, fwd.ctypes.data_as(vp), fwd.size, inv.ctypes.data_as(vp), inv.size,
                                  ctypes.byref(nf), ctypes.byref(ni)), "vocab_tables")
    return fwd, inv


class Vocab:
    """merges (k, 2) uint32; byte_ids (256), merge_ids (k), special_ids (len(specials)) uint32: the vocabulary
    id of every byte, merge and special; specials: list of bytes; rule: a preset name of api.SPLIT_PRESETS"""

    def __init__(self, merges, byte_ids, merge_ids, special_ids, specials, rule):
        self.merges = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1, 2)
        self.byte_ids = np.ascontiguousarray(byte_ids, dtype=np.uint32).reshape(-1)
        self.merge_ids = np.ascontiguousarray(merge_ids, dtype=np.uint32).reshape(-1)
        self.special_ids = np.ascontiguousarray(special_ids, dtype=np.uint32).reshape(-1)
        self.specials = [bytes(s) for s in specials]
        self.rule = rule
        if rule not in api.SPLIT_PRESETS:
            raise BpeError(f"vocabulary: no preset {rule!r} (have {sorted(api.SPLIT_PRESETS)})")
        if self.byte_ids.size != 256 or self.special_ids.size != len(self.specials):
            raise BpeError("vocabulary: 256 byte ids and one id per special are needed")
        self._c = None
        self.check()

    def __eq__(self, other):
        return (isinstance(other, Vocab) and self.rule == other.rule and self.specials == other.specials and
                all(np.array_equal(getattr(self, k), getattr(other, k))
                    for k in ("merges", "byte_ids", "merge_ids", "special_ids")))

    def __repr__(self):
        return f"Vocab(rule={self.rule!r}, merges={self.merges.shape[0]}, specials={len(self.specials)})"

    def c_vocab(self):
        if self._c is None:
            self._c = _CVocab(self)
        return self._c

    def check(self):
        """raise BpeError unless the numbering is one the engine takes (bpe_ex.h bpe_vocab_check: ids pairwise
        distinct and below 2^24, every merge made of earlier ids, the counts in agreement) and the specials
        are a set the split takes (api.check_specials)"""
        if self.specials:
            api.check_specials(self.specials)
        msg = ctypes.create_string_buffer(400)
        m = np.ascontiguousarray(self.merges.reshape(-1))
        rc = _lib.load().bpe_vocab_check(self.c_vocab().ref, m.ctypes.data_as(ctypes.c_void_p) if m.size else None,
                                         self.merges.shape[0], msg, len(msg))
        if rc:
            raise BpeError(msg.value.decode(errors="replace") or f"vocabulary: refused ({rc})")

    @property
    def size(self):
        """the largest vocabulary id + 1"""
        return int(max(self.byte_ids.max(), self.merge_ids.max(initial=0), self.special_ids.max(initial=0))) + 1

    def token_bytes(self):
        """the bytes of every byte and merge token by internal id (256 + merges entries)"""
        out = [bytes([b]) for b in range(256)]
        for a, b in self.merges.tolist():
            out.append(out[a] + out[b])
        return out

    # ---------------------------------------------------------------- construction

    @classmethod
    def from_merges(cls, merges, rule, specials=()):
        """the identity numbering of a list trained here: byte b is b, merge r is 256 + r, special j follows"""
        m = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1, 2)
        k, s = m.shape[0], len(specials)
        return cls(m, np.arange(256), 256 + np.arange(k), 256 + k + np.arange(s), specials, rule)

    @classmethod
    def _assemble(cls, tokens, merges, specials, rule, where):
        """tokens: {bytes: id} of the model's vocabulary; merges: [(bytes, bytes)] in rank order; specials:
        [(bytes, id)].  Numbers the merges, checks reachability and returns the Vocab."""
        special_ids = {i for _, i in specials}
        internal = {}
        byte_ids = np.zeros(256, dtype=np.uint32)
        for b in range(256):
            t = bytes([b])
            if t not in tokens:
                raise BpeError(f"{where}: byte 0x{b:02x} has no token: not a byte-level vocabulary")
            byte_ids[b] = tokens[t]
            internal[t] = b
        pairs, merge_ids, rank = [], [], {}
        for r, (x, y) in enumerate(merges):
            if x not in internal or y not in internal:
                raise BpeError(f"{where}: merge {r} ({x!r} + {y!r}) names a token that no earlier merge makes")
            z = x + y
            if z in internal:
                raise BpeError(f"{where}: merge {r} ({x!r} + {y!r}) makes a token that exists already")
            if z not in tokens:
                raise BpeError(f"{where}: merge {r} makes {z!r}, which the vocabulary does not list")
            pairs.append((internal[x], internal[y]))
            merge_ids.append(tokens[z])
            rank[pairs[-1]] = r
            internal[z] = 256 + r
        # reachability: every listed token is a byte, a merge result or a special, and replays to its id
        bad = []
        for t, i in tokens.items():
            if i in special_ids:
                continue
            if t not in internal or replay(list(t), rank) != [internal[t]]:
                bad.append((i, t))
        if bad:
            bad.sort()
            first = ", ".join(f"{t!r} (id {i})" for i, t in bad[:5])
            raise BpeError(f"{where}: {len(bad)} token(s) cannot be reached by the merges from their bytes: {first}"
                           f"{', ...' if len(bad) > 5 else ''}")
        return cls(np.array(pairs, dtype=np.uint32).reshape(-1, 2), byte_ids, merge_ids, [i for _, i in specials],
                   [s for s, _ in specials], rule)

    @classmethod
    def from_tokenizer_json(cls, path):
        """read a byte-level BPE tokenizer.json.  The rule comes from its pre-tokenizer (ByteLevel with
        use_regex: "gpt2_unicode"; Sequence[Split(the cl100k pattern, Isolated), ByteLevel(use_regex false)]:
        "cl100k"), the specials from added_tokens.  Refused, by name: add_prefix_space, a normalizer,
        byte_fallback, dropout, a subword prefix or suffix, an added token with lstrip / rstrip / single_word /
        normalized, any other pre-tokenizer or pattern, a model type other than BPE, and a vocabulary with a
        token its merges do not reach.  A post-processor (Llama 3's adds <|begin_of_text|>) is not applied:
        the ids are those of `tokenizers` with add_special_tokens=False (Tokenizer.encode_packed takes a BOS and
        an EOS by name)."""
        where = str(path)
        with open(path, encoding="utf-8") as f:
            j = json.load(f)
        model = j.get("model") or {}
        if model.get("type", "BPE") != "BPE":
            raise BpeError(f"{where}: model type {model.get('type')!r}, only BPE is read")
        if j.get("normalizer") is not None:
            raise BpeError(f"{where}: a normalizer ({j['normalizer'].get('type')!r}) is not supported")
        if model.get("byte_fallback"):
            raise BpeError(f"{where}: byte_fallback is not supported")
        if model.get("dropout"):
            raise BpeError(f"{where}: dropout ({model['dropout']}) is not supported")
        for key in ("continuing_subword_prefix", "end_of_word_suffix"):
            if model.get(key):
                raise BpeError(f"{where}: {key} ({model[key]!r}) is not supported")
        rule = cls._rule_of(j.get("pre_tokenizer"), where)
        specials = []
        for t in j.get("added_tokens") or []:
            for key in ("lstrip", "rstrip", "single_word", "normalized"):
                if t.get(key):
                    raise BpeError(f"{where}: added token {t.get('content')!r} has {key} set, which is not supported")
            specials.append((t["content"].encode("utf-8"), int(t["id"])))
        special_by_id = {i: s for s, i in specials}
        tokens = {}
        for text, i in (model.get("vocab") or {}).items():
            if i in special_by_id:  # (GPT-2 lists <|endoftext|> in the model's vocabulary too)
                if text.encode("utf-8") != special_by_id[i] and _from_alphabet(text, f"{where}: token") != special_by_id[i]:
                    raise BpeError(f"{where}: id {i} is both the token {text!r} and the added token {special_by_id[i]!r}")
                continue
            tokens[_from_alphabet(text, f"{where}: token")] = int(i)
        merges = []
        for r, m in enumerate(model.get("merges") or []):
            parts = m.split(" ") if isinstance(m, str) else list(m)
            if len(parts) != 2:
                raise BpeError(f"{where}: merge {r} ({m!r}) is not a pair")
            merges.append(tuple(_from_alphabet(p, f"{where}: merge {r}: part") for p in parts))
        return cls._assemble(tokens, merges, specials, rule, where)

    @staticmethod
    def _rule_of(pt, where):
        def refuse(what):
            raise BpeError(f"{where}: {what}: pre-tokenizer {json.dumps(pt)} is not supported (ByteLevel with "
                           f"use_regex, or Split on the cl100k pattern followed by ByteLevel without, are)")

        def byte_level(p, regex):
            if p.get("type") != "ByteLevel":
                refuse(f"{p.get('type')!r} where ByteLevel is expected")
            if p.get("add_prefix_space"):
                raise BpeError(f"{where}: add_prefix_space is not supported")
            if bool(p.get("use_regex", True)) != regex:
                refuse(f"ByteLevel with use_regex {p.get('use_regex', True)!r}")

        if not isinstance(pt, dict):
            refuse("no pre-tokenizer")
        if pt.get("type") == "ByteLevel":
            byte_level(pt, True)
            return "gpt2_unicode"
        if pt.get("type") == "Sequence":
            seq = pt.get("pretokenizers") or []
            if len(seq) != 2 or seq[0].get("type") != "Split":
                refuse("a Sequence other than [Split, ByteLevel]")
            sp = seq[0]
            pattern = (sp.get("pattern") or {}).get("Regex")
            if pattern != CL100K_PATTERN:
                refuse(f"the pattern {pattern!r}")
            if sp.get("behavior") != "Isolated" or sp.get("invert"):
                refuse(f"Split with behavior {sp.get('behavior')!r}, invert {sp.get('invert')!r}")
            byte_level(seq[1], False)
            return "cl100k"
        refuse(f"type {pt.get('type')!r}")

    @classmethod
    def from_tiktoken(cls, path, rule, specials=None):
        """read a rank file: per line a base64 token, a space and its rank (its id).  specials: {bytes: id}.
        The merges are derived in rank order: a token of two or more bytes is replayed with the merges found so
        far, must come out as exactly two ids, and those are its merge."""
        where = str(path)
        if rule not in RULES:
            raise BpeError(f"{where}: rule {rule!r}: a rank file goes with one of {RULES}")
        ranked = []
        with open(path, "rb") as f:
            for ln, line in enumerate(f, 1):
                if not line.strip():
                    continue
                try:
                    tok, r = line.split()
                    ranked.append((int(r), base64.b64decode(tok, validate=True)))
                except ValueError:
                    raise BpeError(f"{where}:{ln}: not a base64 token and a rank") from None
        ranked.sort()
        tokens = {}
        for r, t in ranked:
            if t in tokens or not t:
                raise BpeError(f"{where}: the token {t!r} is listed twice or empty")
            tokens[t] = r
        by_id = [bytes([b]) for b in range(256)]  # the bytes of every internal id so far
        rank, merges, bad = {}, [], []
        for r, t in ranked:
            if len(t) < 2:
                continue
            parts = replay(list(t), rank)
            if len(parts) != 2:
                bad.append((r, t))
                continue
            rank[(parts[0], parts[1])] = len(merges)
            merges.append((by_id[parts[0]], by_id[parts[1]]))
            by_id.append(t)
        if bad:
            first = ", ".join(f"{t!r} (rank {r})" for r, t in bad[:5])
            raise BpeError(f"{where}: {len(bad)} token(s) cannot be reached by the merges from their bytes: {first}"
                           f"{', ...' if len(bad) > 5 else ''}")
        sp = sorted((specials or {}).items(), key=lambda kv: kv[1])
        return cls._assemble(tokens, merges, [(bytes(s), int(i)) for s, i in sp], rule, where)

    # ---------------------------------------------------------------- export

    def to_tiktoken(self, path):
        """write the byte and merge tokens as a rank file (the specials are not part of that format).  In a rank
        file a token's id is also its priority, so only a vocabulary whose merge ids grow with the rank has one."""
        if (np.diff(self.merge_ids.astype(np.int64)) <= 0).any():
            raise BpeError("to_tiktoken: the merge ids do not grow with the rank: a rank file cannot say this order")
        rows = sorted(zip(list(self.byte_ids) + list(self.merge_ids), self.token_bytes()))
        with open(path, "wb") as f:
            for i, t in rows:
                f.write(base64.b64encode(t) + b" " + str(int(i)).encode() + b"\n")

    def to_tokenizer_json(self, path):
        """write the vocabulary as a tokenizer.json that from_tokenizer_json and `tokenizers` read: a byte-level
        BPE model, the rule's pre-tokenizer, the specials as added tokens (listed in the model's vocabulary
        as well, which is what makes `tokenizers` keep their ids)"""
        if self.rule not in RULES:
            raise BpeError(f"to_tokenizer_json: rule {self.rule!r} has no tokenizer.json form (only {RULES} have)")
        byte_level = {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True}
        if self.rule == "gpt2_unicode":
            pre = dict(byte_level, use_regex=True)
        else:
            pre = {"type": "Sequence", "pretokenizers": [
                {"type": "Split", "pattern": {"Regex": CL100K_PATTERN}, "behavior": "Isolated", "invert": False},
                dict(byte_level, use_regex=False)]}
        tb = self.token_bytes()
        text = [_to_alphabet(t) for t in tb]
        vocab = {text[k]: int(i) for k, i in enumerate(list(self.byte_ids) + list(self.merge_ids))}
        added = []
        for s, i in zip(self.specials, self.special_ids):
            try:
                content = s.decode("utf-8")
            except UnicodeDecodeError:
                raise BpeError(f"to_tokenizer_json: the special {s!r} is not UTF-8") from None
            if content in vocab:
                raise BpeError(f"to_tokenizer_json: the special {s!r} reads like a token of the vocabulary")
            vocab[content] = int(i)
            added.append({"id": int(i), "content": content, "single_word": False, "lstrip": False, "rstrip": False,
                          "normalized": False, "special": True})
        doc = {"version": "1.0", "truncation": None, "padding": None, "added_tokens": added, "normalizer": None,
               "pre_tokenizer": pre, "post_processor": None, "decoder": dict(byte_level, use_regex=True),
               "model": {"type": "BPE", "dropout": None, "unk_token": None, "continuing_subword_prefix": None,
                         "end_of_word_suffix": None, "fuse_unk": False, "byte_fallback": False, "ignore_merges": False,
                         "vocab": dict(sorted(vocab.items(), key=lambda kv: kv[1])),
                         "merges": [f"{text[a]} {text[b]}" for a, b in self.merges.tolist()]}}
        with open(path, "w", encoding="utf-8") as f:
            json.dump(doc, f, ensure_ascii=False)


class Tokenizer:
    """Encode to and decode from a vocabulary's own ids on one GPU: the split of vocab.rule around
    vocab.specials, the merges applied inside the pieces, the ids rewritten on the device."""

    def __init__(self, vocab, device=0):
        self.vocab = vocab
        self.device = int(device)
        self._engine = None

    def _eng(self):
        if self._engine is None:
            self._engine = api.Engine(self.device)
        return self._engine

    def close(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None

    @staticmethod
    def _spans_unit(return_spans, what):
        if return_spans not in (None, "byte", "char"):
            raise BpeError(f"{what}: return_spans {return_spans!r} (None, \"byte\" or \"char\")")
        return return_spans

    def _spans(self, unit):
        v = self.vocab
        return self._eng().token_spans(v.merges, v.specials or None, vocab=v, unit=unit)

    def encode(self, data, return_offsets=False, return_spans=None):
        """uint32 vocabulary ids of data (bytes; a str is encoded as UTF-8).  return_offsets: also the id and
        byte offsets of the pieces, as api.encode_split returns them.  return_spans ("byte" or "char"): also, as
        the last element of the result, the span of every id in data, uint32[ids, 2], computed on the device: in
        bytes, or in characters as Encoding.offsets of the `tokenizers` library counts them for a tokenizer.json
        without a post-processor (a token that holds a part of a character reports the whole character;
        trim_offsets belongs to a ByteLevel post-processor, which a Vocab does not apply)."""
        unit = self._spans_unit(return_spans, "encode")
        if isinstance(data, str):
            data = data.encode("utf-8")
        e, v = self._eng(), self.vocab
        e.load(data)
        e.split(v.rule, v.specials or None)
        e.encode_split(v.merges)
        e.map_ids(v)
        ids = e.ids()
        out = (ids, e.doc_offsets(), e.split_offsets()) if return_offsets else (ids,)
        if unit is not None:
            out += (self._spans(unit),)
        return out if len(out) > 1 else ids

    def encode_batch(self, texts, max_length=None, pad_id=None, truncation_side="right", return_tensors=None,
                     return_spans=None):
        """Encode a list of texts (bytes; a str is encoded as UTF-8) in one pass, each exactly as encode() does it
        alone: no piece, special or merge reaches from one text into the next, and an empty text has no id.
        Without max_length: (ids, text_off), text k's ids being ids[text_off[k]:text_off[k + 1]] (text_off uint64,
        len(texts) + 1 entries).  With max_length: (rows, lens), uint32[texts, max_length] and uint32[texts]: a
        longer text is cut at truncation_side ("right" keeps its first ids, "left" its last), pad_id fills the row
        behind the ids (required; any uint32, not checked against the vocabulary), lens[k] counts the ids in row
        k.  return_tensors="pt" (with max_length): torch int32 tensors on the tokenizer's device, filled on the
        device without fetching the ids to the host.  return_spans ("byte" or "char", see encode()): a third
        element, every span relative to its own text: without max_length the spans uint32[ids, 2]; with it
        span_rows uint32[texts, max_length, 2], cut as the rows are, (0, 0) behind the ids, and with
        truncation_side "left" still relative to the whole text; with return_tensors="pt" a torch int32 tensor
        filled on the device (no id and no span passes through the host; a batch with a text of 2^31 bytes or
        more is refused, since int32 could not hold its spans)."""
        unit = self._spans_unit(return_spans, "encode_batch")
        if return_tensors not in (None, "pt"):
            raise BpeError(f"encode_batch: return_tensors {return_tensors!r} (None or \"pt\")")
        if max_length is None and (return_tensors is not None or pad_id is not None):
            raise BpeError("encode_batch: pad_id and return_tensors go with max_length")
        if max_length is not None and pad_id is None:
            raise BpeError("encode_batch: max_length needs a pad_id")
        if return_tensors == "pt":  # (before any work: the tensors must be possible)
            import torch
            if not torch.cuda.is_available():
                # (a PyTorch-ROCm wheel carries a HIP runtime of its own; of two runtimes in a process the one loaded
                # first owns the GPU, and this library binds to torch's only when torch was there before it)
                raise BpeError('encode_batch: return_tensors="pt": torch sees no GPU; import torch before the first '
                               "call into llmtokenizer_amd, so that both share one HIP runtime")
            if unit is not None:
                for k, t in enumerate(texts):
                    # (a str of fewer than 2^29 characters has fewer than 2^31 bytes: only a longer one is encoded here)
                    if len(t) >= 1 << 29 and len(t.encode("utf-8") if isinstance(t, str) else t) >= 1 << 31:
                        raise BpeError(f'encode_batch: return_tensors="pt" with return_spans: text {k} holds 2^31 bytes '
                                       "or more, its spans do not fit int32")
        e, v = self._eng(), self.vocab
        n_texts = e.load_texts(texts)
        e.split(v.rule, v.specials or None)
        e.encode_split(v.merges)
        e.map_ids(v)
        if max_length is None:
            out = (e.ids(), e.text_offsets())
            return out + (self._spans(unit),) if unit is not None else out
        if unit is not None:  # (kept on the device; only the rows below fetch them)
            pairs, k, sp, cv, keep = api._span_args(v.merges, v.specials or None, v)
            _lib.check(e.L.bpe_gpu_token_spans(e.ctx, pairs, k, sp, cv, api.SPAN_UNITS[unit]), "token_spans")
        if return_tensors is None:
            out = e.pack_texts(max_length, pad_id, truncation_side)
            return out + (e.pack_spans(max_length, truncation_side),) if unit is not None else out
        dev = torch.device("cuda", self.device)
        rows = torch.empty((n_texts, int(max_length)), dtype=torch.int32, device=dev)
        out = e.pack_texts(max_length, pad_id, truncation_side, out=rows)
        if unit is None:
            return out
        span_rows = torch.empty((n_texts, int(max_length), 2), dtype=torch.int32, device=dev)
        return out + (e.pack_spans(max_length, truncation_side, out=span_rows),)

    def _special_id(self, tok, what, fn="encode_packed"):
        """the id of a BOS / EOS argument: None, an int (a vocabulary id) or the name of one of vocab.specials"""
        if tok is None or isinstance(tok, (int, np.integer)):
            return None if tok is None else int(tok)
        name = tok.encode("utf-8") if isinstance(tok, str) else bytes(tok)
        specials = [bytes(s) for s in self.vocab.specials]
        if name not in specials:
            raise BpeError(f"{fn}: {what} {tok!r} is none of the vocabulary's specials")
        return int(self.vocab.special_ids[specials.index(name)])

    def encode_packed(self, texts, seq_len, pad_id, bos=None, eos=None, drop_last=False, return_segments=False,
                      return_positions=False, return_tensors=None):
        """Encode a list of texts as encode_batch() does and lay the ids out for training (Engine.pack_stream; the
        contract: bpe_gpu.h, "Packed streams"): every text wrapped in bos / eos (None: without; an int is taken as
        a vocabulary id, a str or bytes must be one of vocab.specials and stands for its id), the texts joined end to
        end and cut into rows of exactly seq_len ids.  Nothing is truncated; the last row is filled with pad_id (any
        uint32, not checked against the vocabulary) or, with drop_last, dropped unless full.  Returns
        (rows[, seg][, pos], N): uint32[R, seq_len] arrays, seg (return_segments) the index of every cell's text in
        the batch, 0xFFFFFFFF in a pad cell, pos (return_positions) the cell's position in its text's stretch of the
        row, and N the cells of the stream (rows.reshape(-1)[:N] is the stream, the rest pad).
        return_tensors="pt": torch int32 tensors on the tokenizer's device, filled on the device without fetching the
        ids to the host (a pad cell's seg reads -1)."""
        if return_tensors not in (None, "pt"):
            raise BpeError(f"encode_packed: return_tensors {return_tensors!r} (None or \"pt\")")
        bos_id, eos_id = self._special_id(bos, "bos"), self._special_id(eos, "eos")
        api.check_stream(seq_len, pad_id, bos_id, eos_id, drop_last)  # (before any work)
        if return_tensors == "pt":
            import torch
            if not torch.cuda.is_available():  # (see encode_batch)
                raise BpeError('encode_packed: return_tensors="pt": torch sees no GPU; import torch before the first '
                               "call into llmtokenizer_amd, so that both share one HIP runtime")
        e, v = self._eng(), self.vocab
        e.load_texts(texts)
        e.split(v.rule, v.specials or None)
        e.encode_split(v.merges)
        e.map_ids(v)
        R, N = e.stream_rows(seq_len, bos_id, eos_id, drop_last)
        if return_tensors is None:
            out = e.pack_stream(seq_len, pad_id, bos_id, eos_id, drop_last, return_segments, return_positions)
            return (out if isinstance(out, tuple) else (out,)) + (N,)
        dev = torch.device("cuda", self.device)
        new = lambda: torch.empty((R, int(seq_len)), dtype=torch.int32, device=dev)  # noqa: E731
        out = e.pack_stream(seq_len, pad_id, bos_id, eos_id, drop_last,
                            out=(new(), new() if return_segments else None, new() if return_positions else None))
        return tuple(t for t in out if t is not None) + (N,)

    def decode_rows(self, rows, lens=None, pad_id=None, eos=None, skip_specials=False, return_bounds=False):
        """The texts of a [B, L] grid of ids as a model hands it back: a list of B bytes objects (NUL bytes dropped, as
        decode does).  rows: a 2-D numpy array of uint32, int32, int64 or uint64, or a torch tensor of int32 or int64
        on the tokenizer's device with stride(1) == 1 and stride(0) >= shape[1], such as out[:, P:] of what generate
        returned: it is read where it lies and no id passes through the host (Engine.unpack_rows; the contract:
        bpe_gpu.h, "Rows back to texts").  Row k's window is its first lens[k] cells (lens None: the whole row).  Its
        text begins behind the leading cells equal to pad_id (None: at the first cell) and ends before the first cell
        that is an eos id or pad_id, or at the window's end; so left-padded rows with pad_id == eos read as they are
        meant, and a text whose first token is the pad id loses it.  eos: None, an int (a vocabulary id), the name of
        one of vocab.specials (str or bytes), or a list of up to 8 of them.  skip_specials: the ids of vocab.specials
        are left out of the text.  A cell outside the text is never judged, whatever it holds; an id inside it that
        the vocabulary does not hold raises BpeError.  return_bounds: also bounds uint32[B, 2], every row's (start,
        end) in cells: end - start is the length of what the row generated."""
        many = isinstance(eos, (list, tuple)) or (isinstance(eos, np.ndarray) and eos.ndim)
        stops = [self._special_id(t, "eos", "decode_rows") for t in (eos if many else [eos]) if t is not None]
        if hasattr(rows, "data_ptr"):  # a torch tensor
            import torch
            if not torch.cuda.is_available():  # (see encode_batch)
                raise BpeError("decode_rows: a torch tensor: torch sees no GPU; import torch before the first "
                               "call into llmtokenizer_amd, so that both share one HIP runtime")
        e, v = self._eng(), self.vocab
        B, _ = e._unpack_rows(rows, lens, pad_id, stops, v.special_ids if skip_specials else None)
        out, bo = e.decode_rows(v.merges, v.specials or None, vocab=v)
        texts = [out[int(bo[k]):int(bo[k + 1])] for k in range(B)]
        return (texts, e.fetch_rows()[2]) if return_bounds else texts

    def decode_batch(self, ids, text_off):
        """the inverse of encode_batch(texts): the list of the texts' bytes (NUL bytes dropped, as decode does)"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        off = np.ascontiguousarray(text_off, dtype=np.uint64).reshape(-1)
        v = self.vocab
        out, bo = self._eng().decode_docs(ids, off, v.merges, v.specials or None, vocab=v)
        return [out[int(bo[k]):int(bo[k + 1])] for k in range(off.size - 1)]

    def decode(self, ids):
        """the bytes of vocabulary ids (NUL bytes dropped, as api.decode_batch does); an id the vocabulary does
        not hold raises BpeError"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        v = self.vocab
        out, _ = self._eng().decode_docs(ids, [0, ids.size], v.merges, v.specials or None, vocab=v)
        return out
