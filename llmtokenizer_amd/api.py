"""Python mirror of the drop-in C API (include/bpe.h + bpe_ex.h), over ctypes.

Names and argument meaning follow the reference (neofytr/LLMTokenizer
bpe/inc/bpe.h): compress(path) trains until the reference's stop rule and
returns (merges, ids); decompress(ids, merges) inverts it; dump_pairs /
read_pairs use the reference's raw 8-byte record format.  Merges are numpy
uint32 arrays of shape (k, 2) for ids 256..255+k.  Every call runs through
libbpe_amd.so on the GPU; errors raise BpeError (the C layer returns NULL).
"""
import ctypes
import os
import weakref

import numpy as np

from . import _lib
from ._lib import BpeError, GpuStats  # noqa: F401

_u32p = ctypes.POINTER(ctypes.c_uint32)


def _arr_to_merges(arr_p):
    """dyn_arr_t* of pair_t (ids 0..last_index) -> (k,2) uint32 for ids >= 256"""
    L = _lib.load()
    last = arr_p.contents.last_index
    k = max(0, last - 255)
    out = np.zeros((k, 2), dtype=np.uint32)
    buf = (ctypes.c_uint32 * 2)()
    for r in range(k):
        if not L.dyn_arr_get(arr_p, 256 + r, ctypes.cast(buf, ctypes.c_void_p)):
            raise BpeError(f"merge list has no record for id {256 + r}")
        out[r] = (buf[0], buf[1])
    return out


def _merges_to_arr(merges):
    L = _lib.load()
    m = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1, 2)
    arr = L.dyn_arr_create(512, 8)
    if not arr:
        raise MemoryError
    buf = (ctypes.c_uint32 * 2)()
    for i in range(256):
        buf[0], buf[1] = i, 0
        L.dyn_arr_set(arr, i, ctypes.cast(buf, ctypes.c_void_p))
    for r in range(m.shape[0]):
        buf[0], buf[1] = int(m[r, 0]), int(m[r, 1])
        L.dyn_arr_set(arr, 256 + r, ctypes.cast(buf, ctypes.c_void_p))
    return arr


def _take_ids(ptr, n):
    """the library's malloc'd id buffer as a numpy array without a copy (a
    multi-GB encoding): freed when the array (and every view of it) is gone"""
    addr = ctypes.cast(ptr, ctypes.c_void_p).value
    if not n:
        ctypes.CDLL(None).free(ctypes.c_void_p(addr))
        return np.zeros(0, dtype=np.uint32)
    ids = np.ctypeslib.as_array(ptr, shape=(n,))
    weakref.finalize(ids, ctypes.CDLL(None).free, ctypes.c_void_p(addr))
    return ids


def release_engines():
    """free the engine contexts compress() & co. keep between calls
    (bpe_ex.h bpe_release_engines; also run at interpreter exit)"""
    _lib.load().bpe_release_engines()


def last_stats():
    st = GpuStats()
    _lib.load().bpe_last_stats(ctypes.byref(st))
    return st.as_dict()


def compress(path, max_merges=None, device=0):
    """Train on a file (reference compress, bpe.c:541).  Returns (merges, ids)."""
    L = _lib.load()
    enc = _u32p()
    n = ctypes.c_size_t(0)
    if max_merges is None and device == 0:
        # the C entry point itself reads BPE_MAX_MERGES / BPE_DEVICE / BPE_NUM_GPUS / BPE_DEVICES
        arr = L.compress(os.fsencode(path), ctypes.byref(enc), ctypes.byref(n))
    else:
        mm = -1 if max_merges is None else int(max_merges)
        arr = L.compress_ex(os.fsencode(path), mm, int(device), ctypes.byref(enc), ctypes.byref(n))
    if not arr:
        raise BpeError(f"compress({path!r}) failed")
    try:
        merges = _arr_to_merges(arr)
    finally:
        L.dyn_arr_free(arr)
    return merges, _take_ids(enc, n.value)


def train_bytes(data: bytes, max_merges=-1, device=0):
    """Train on in-memory bytes (no NUL truncation here).  Returns (merges, ids)."""
    L = _lib.load()
    buf = np.frombuffer(data, dtype=np.uint8)
    enc = _u32p()
    n = ctypes.c_size_t(0)
    arr = L.bpe_train_bytes(buf.ctypes.data_as(ctypes.c_void_p), buf.size, int(max_merges), int(device),
                            ctypes.byref(enc), ctypes.byref(n))
    if not arr:
        raise BpeError("bpe_train_bytes failed")
    try:
        merges = _arr_to_merges(arr)
    finally:
        L.dyn_arr_free(arr)
    return merges, _take_ids(enc, n.value)


def train_bytes_devices(data: bytes, devices, max_merges=-1):
    """One training job over len(devices) devices in this process (bpe_train_bytes_devices:
    contiguous shards, one host thread per device; a device may repeat).  Returns (merges, ids)."""
    L = _lib.load()
    buf = np.frombuffer(data, dtype=np.uint8)
    devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
    enc = _u32p()
    n = ctypes.c_size_t(0)
    arr = L.bpe_train_bytes_devices(buf.ctypes.data_as(ctypes.c_void_p), buf.size, int(max_merges), len(devices),
                                    devs, ctypes.byref(enc), ctypes.byref(n))
    if not arr:
        raise BpeError("bpe_train_bytes_devices failed")
    try:
        merges = _arr_to_merges(arr)
    finally:
        L.dyn_arr_free(arr)
    return merges, _take_ids(enc, n.value)


def encode(data: bytes, merges, device=0):
    """Standalone encoder: merges applied in rank order (reference replace pass)."""
    L = _lib.load()
    buf = np.frombuffer(data, dtype=np.uint8)
    arr = _merges_to_arr(merges)
    n = ctypes.c_size_t(0)
    try:
        p = L.bpe_encode_bytes(buf.ctypes.data_as(ctypes.c_void_p), buf.size, arr, int(device), ctypes.byref(n))
    finally:
        L.dyn_arr_free(arr)
    if not p:
        raise BpeError("bpe_encode_bytes failed")
    return _take_ids(p, n.value)


def _doc_offsets(offsets):
    return np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)


def encode_batch(docs, merges, device=0):
    """Encode a batch of documents (bytes-like objects) in one pass: no merge
    crosses a document boundary.  Returns (ids, offsets): ids[offsets[d]:offsets[d + 1]]
    equals encode(docs[d], merges); offsets is uint64 of length len(docs) + 1."""
    L = _lib.load()
    docs = [bytes(d) for d in docs]
    buf = np.frombuffer(b"".join(docs), dtype=np.uint8)
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.fromiter((len(d) for d in docs), dtype=np.uint64, count=len(docs)))
    arr = _merges_to_arr(merges)
    n = ctypes.c_size_t(0)
    ido = ctypes.POINTER(ctypes.c_uint64)()
    try:
        p = L.bpe_encode_docs(buf.ctypes.data_as(ctypes.c_void_p), buf.size, off.ctypes.data_as(ctypes.c_void_p),
                              len(docs), arr, int(device), ctypes.byref(n), ctypes.byref(ido))
    finally:
        L.dyn_arr_free(arr)
    if not p:
        raise BpeError("bpe_encode_docs failed")
    offsets = np.ctypeslib.as_array(ido, shape=(len(docs) + 1,)).copy()
    ctypes.CDLL(None).free(ctypes.cast(ido, ctypes.c_void_p))
    return _take_ids(p, n.value), offsets


# bpe_gpu.h BPE_SPLIT_LINES / BPE_SPLIT_WORDS / BPE_SPLIT_GPT2 / BPE_SPLIT_GPT2_UNICODE / BPE_SPLIT_CL100K (3 and 5 are no presets)
SPLIT_PRESETS = {"lines": 0, "words": 1, "gpt2": 2, "gpt2_unicode": 4, "cl100k": 6}
TABLE_PRESETS = ("lines", "words")  # the presets two tables express


def _no_tables(rule):
    """is rule the name of a preset without tables ("gpt2", "gpt2_unicode", "cl100k": the preset calls run them)?"""
    return isinstance(rule, str) and rule in SPLIT_PRESETS and rule not in TABLE_PRESETS


UNICODE_CLASSES = ("P", "L", "N", "S", "W")


def unicode_class(cp):
    """The class of code point cp under "gpt2_unicode" (bpe_ex.h bpe_unicode_class): "L" \\p{L}, "N" \\p{N},
    "S" U+0020, "W" the other White_Space, "P" the rest (and everything above U+10FFFF).  No GPU."""
    return UNICODE_CLASSES[_lib.load().bpe_unicode_class(int(cp))]


def unicode_info():
    """{"source", "digest"}: where the committed class table came from ("regex <version>") and the FNV-1a 64
    of the 0x110000 classes as bytes 0 P, 1 L, 2 N, 3 S, 4 W (bpe_ex.h bpe_unicode_info).  No GPU."""
    src, dig = ctypes.c_char_p(), ctypes.c_uint64(0)
    _lib.check(_lib.load().bpe_unicode_info(ctypes.byref(src), ctypes.byref(dig)), "unicode_info")
    return {"source": src.value.decode(), "digest": int(dig.value)}


def split_rule(preset):
    """The tables (cls uint8[256], brk uint16[16]) of a preset split rule, "lines"
    or "words" (bpe_gpu.h bpe_gpu_split_rule; this project's rules, not GPT-2's
    regular expression): a piece starts at byte i when bit cls[b[i]] of
    brk[cls[b[i - 1]]] is set, and at byte 0.  "gpt2", "gpt2_unicode" and "cl100k" have no
    tables (a start there depends on six and fifteen bytes): pass the name to
    split / encode_split / train_split / split_host."""
    if _no_tables(preset):
        raise BpeError(f'split_rule: the rule "{preset}" has no tables: pass its name as the rule')
    if preset not in TABLE_PRESETS:
        raise BpeError(f"split_rule: no preset {preset!r} (have {sorted(SPLIT_PRESETS)})")
    L = _lib.load()
    cls = np.zeros(256, dtype=np.uint8)
    brk = np.zeros(16, dtype=np.uint16)
    _lib.check(L.bpe_gpu_split_rule(SPLIT_PRESETS[preset], cls.ctypes.data_as(ctypes.c_void_p),
                                    brk.ctypes.data_as(ctypes.c_void_p)), "split_rule")
    return cls, brk


class _Specials:
    """bpe_gpu.h bpe_gpu_specials over a list of bytes-like specials (keeps the buffers it points to)"""

    def __init__(self, specials):
        items = [bytes(s) for s in specials]
        self.blob = np.frombuffer(b"".join(items) + b"\0", dtype=np.uint8)  # (+ a byte: never an empty buffer)
        self.len = np.array([len(s) for s in items] + [0], dtype=np.uint32)
        self.c = _lib.Specials(self.blob.ctypes.data, self.len.ctypes.data, len(items))
        self.ref = ctypes.byref(self.c)


def check_specials(specials):
    """Raise BpeError unless `specials` (a list of bytes-like objects) is a set the split accepts: at most 256
    of 1..64 bytes each, no NUL byte, none a substring of another, no proper suffix of one a prefix of one
    (bpe_gpu.h, "Special tokens"; bpe_ex.h bpe_specials_check).  The message names the pair.  Returns the set as the C calls take it.  No GPU."""
    sp = specials if isinstance(specials, _Specials) else _Specials(specials)
    msg = ctypes.create_string_buffer(400)
    if _lib.load().bpe_specials_check(sp.ref, msg, len(msg)):
        raise BpeError(msg.value.decode(errors="replace"))
    return sp


def _rule_args(rule):
    """(preset or -1, cls pointer, brk pointer, the arrays to keep) of a rule for the *_special calls"""
    if isinstance(rule, str):
        if rule not in SPLIT_PRESETS:
            raise BpeError(f"no preset {rule!r} (have {sorted(SPLIT_PRESETS)})")
        return SPLIT_PRESETS[rule], None, None, None
    cls, brk = _rule_tables(rule)
    return -1, cls.ctypes.data_as(ctypes.c_void_p), brk.ctypes.data_as(ctypes.c_void_p), (cls, brk)


def split_host_special(data: bytes, rule, specials):
    """(offsets, special piece indices, their specials' indices) of the split with specials computed on the
    host in plain C (bpe_ex.h bpe_split_offsets_host_special): the definition Engine.split(rule, specials) is
    held to.  rule: a preset name or a (cls, brk) pair.  No GPU."""
    sp = check_specials(specials)
    L = _lib.load()
    preset, pc, pb, keep = _rule_args(rule)
    buf = np.frombuffer(data, dtype=np.uint8)
    vp = ctypes.c_void_p
    cnt, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.check(L.bpe_split_offsets_host_special(preset, pc, pb, buf.ctypes.data_as(vp), buf.size, sp.ref, None, 0,
                                                ctypes.byref(cnt), None, None, 0, ctypes.byref(m)), "split_host")
    out = np.zeros(cnt.value, dtype=np.uint64)
    piece = np.zeros(max(m.value, 1), dtype=np.uint64)
    index = np.zeros(max(m.value, 1), dtype=np.uint32)
    _lib.check(L.bpe_split_offsets_host_special(preset, pc, pb, buf.ctypes.data_as(vp), buf.size, sp.ref,
                                                out.ctypes.data_as(vp), out.size, ctypes.byref(cnt),
                                                piece.ctypes.data_as(vp), index.ctypes.data_as(vp), m.value,
                                                ctypes.byref(m)), "split_host")
    return out, piece[: m.value], index[: m.value]


def split_host(data: bytes, rule, specials=None):
    """The offsets (uint64: the piece starts followed by len(data)) of a preset
    rule, "lines", "words", "gpt2", "gpt2_unicode" or "cl100k", computed on the host in plain C
    (bpe_ex.h bpe_split_offsets_host): the definition Engine.split(rule) is held
    to.  With specials (a list of bytes-like objects, see check_specials) the
    definition of Engine.split(rule, specials), for a preset or a (cls, brk)
    pair (split_host_special also returns which pieces are specials).  No GPU."""
    if specials is not None:
        return split_host_special(data, rule, specials)[0]
    if not isinstance(rule, str) or rule not in SPLIT_PRESETS:
        raise BpeError(f"split_host: no preset {rule!r} (have {sorted(SPLIT_PRESETS)})")
    L = _lib.load()
    buf = np.frombuffer(data, dtype=np.uint8)
    vp = ctypes.c_void_p
    cnt = ctypes.c_size_t(0)
    _lib.check(L.bpe_split_offsets_host(SPLIT_PRESETS[rule], buf.ctypes.data_as(vp), buf.size, None, 0,
                                        ctypes.byref(cnt)), "split_host")
    out = np.zeros(cnt.value, dtype=np.uint64)
    _lib.check(L.bpe_split_offsets_host(SPLIT_PRESETS[rule], buf.ctypes.data_as(vp), buf.size, out.ctypes.data_as(vp),
                                        out.size, ctypes.byref(cnt)), "split_host")
    return out


def split_info():
    """{"tile", "grid_bytes"}: bytes one workgroup of the split kernels handles per
    step and bytes one grid step covers (bpe_gpu_split_info; for the tests)"""
    out = np.zeros(4, dtype=np.uint64)
    _lib.check(_lib.load().bpe_gpu_split_info(out.ctypes.data_as(ctypes.c_void_p)), "split_info")
    return {"tile": int(out[0]), "grid_bytes": int(out[1])}


def map_info():
    """{"thread", "workgroup", "grid"}: ids one thread of the id-mapping kernels moves per step, ids per
    workgroup step and ids per grid step (bpe_gpu_map_info; for the tests)"""
    out = np.zeros(4, dtype=np.uint64)
    _lib.check(_lib.load().bpe_gpu_map_info(out.ctypes.data_as(ctypes.c_void_p)), "map_info")
    return {"thread": int(out[0]), "workgroup": int(out[1]), "grid": int(out[2])}


def _rule_tables(rule):
    cls, brk = split_rule(rule) if isinstance(rule, str) else rule
    cls = np.ascontiguousarray(cls, dtype=np.uint8).reshape(-1)
    brk = np.ascontiguousarray(brk, dtype=np.uint16).reshape(-1)
    if cls.size != 256 or brk.size != 16:
        raise BpeError("split rule: cls must hold 256 entries and brk 16")
    return cls, brk


def encode_split(data: bytes, merges, rule="words", device=0, specials=None):
    """Split data into pieces on the GPU (rule: a preset name, "lines", "words",
    "gpt2", "gpt2_unicode" or "cl100k" (the pre-tokenizer of cl100k_base and Llama 3), or a (cls, brk) pair, see
    split_rule) and encode the pieces as documents.  Returns (ids,
    id_offsets, byte_offsets), both offsets uint64 of length pieces + 1: piece d
    is data[byte_offsets[d]:byte_offsets[d + 1]] and its ids are
    ids[id_offsets[d]:id_offsets[d + 1]] == encode(piece d, merges).  With specials (a list of
    bytes-like objects, see check_specials) every occurrence of specials[j] is a piece of its own
    with the one id 256 + len(merges) + j."""
    L = _lib.load()
    if specials is not None:
        check_specials(specials)
    gpt2 = _no_tables(rule)
    cls, brk = (None, None) if gpt2 or specials is not None else _rule_tables(rule)
    buf = np.frombuffer(data, dtype=np.uint8)
    arr = _merges_to_arr(merges)
    n, nd = ctypes.c_size_t(0), ctypes.c_size_t(0)
    ido, bo = ctypes.POINTER(ctypes.c_uint64)(), ctypes.POINTER(ctypes.c_uint64)()
    vp = ctypes.c_void_p
    try:
        if specials is not None:
            sp = _Specials(specials)
            preset, pc, pb, keep = _rule_args(rule)
            p = L.bpe_encode_split_special(buf.ctypes.data_as(vp), buf.size, preset, pc, pb, sp.ref, arr, int(device),
                                           ctypes.byref(n), ctypes.byref(ido), ctypes.byref(bo), ctypes.byref(nd))
        elif gpt2:
            p = L.bpe_encode_split_preset(buf.ctypes.data_as(vp), buf.size, SPLIT_PRESETS[rule], arr, int(device),
                                          ctypes.byref(n), ctypes.byref(ido), ctypes.byref(bo), ctypes.byref(nd))
        else:
            p = L.bpe_encode_split(buf.ctypes.data_as(vp), buf.size, cls.ctypes.data_as(vp), brk.ctypes.data_as(vp),
                                   arr, int(device), ctypes.byref(n), ctypes.byref(ido), ctypes.byref(bo),
                                   ctypes.byref(nd))
    finally:
        L.dyn_arr_free(arr)
    if not p:
        raise BpeError("bpe_encode_split failed")
    id_off = np.ctypeslib.as_array(ido, shape=(nd.value + 1,)).copy()
    byte_off = np.ctypeslib.as_array(bo, shape=(nd.value + 1,)).copy()
    ctypes.CDLL(None).free(ctypes.cast(ido, vp))
    ctypes.CDLL(None).free(ctypes.cast(bo, vp))
    return _take_ids(p, n.value), id_off, byte_off


def train_split(data: bytes, rule="words", max_merges=-1, device=0, specials=None):
    """Split data into pieces on the GPU (rule as in encode_split) and train on the
    pieces: merges that never cross a piece boundary, so encode_split with the same
    rule can apply every one of them (bpe_ex.h bpe_train_split).  Returns the
    merges, (k, 2) uint32 for ids 256..255+k.  With specials (see encode_split) their
    occurrences are pieces that take no part in the training."""
    L = _lib.load()
    buf = np.frombuffer(data, dtype=np.uint8)
    vp = ctypes.c_void_p
    if specials is not None:
        check_specials(specials)
        sp = _Specials(specials)
        preset, pc, pb, keep = _rule_args(rule)
        arr = L.bpe_train_split_special(buf.ctypes.data_as(vp), buf.size, preset, pc, pb, sp.ref, int(max_merges),
                                        int(device))
    elif _no_tables(rule):
        arr = L.bpe_train_split_preset(buf.ctypes.data_as(vp), buf.size, SPLIT_PRESETS[rule], int(max_merges),
                                       int(device))
    else:
        cls, brk = _rule_tables(rule)
        arr = L.bpe_train_split(buf.ctypes.data_as(vp), buf.size, cls.ctypes.data_as(vp), brk.ctypes.data_as(vp),
                                int(max_merges), int(device))
    if not arr:
        raise BpeError("bpe_train_split failed")
    try:
        return _arr_to_merges(arr)
    finally:
        L.dyn_arr_free(arr)


def decode_batch(ids, offsets, merges, device=0, specials=None):
    """Inverse of encode_batch: the list of the documents' bytes (NUL bytes dropped, as decompress does).
    With specials (see encode_split) the id 256 + len(merges) + j is specials[j]."""
    L = _lib.load()
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    off = _doc_offsets(offsets)
    if off.size < 1:
        raise BpeError("decode_batch: offsets must hold len(docs) + 1 entries")
    if specials is not None:
        check_specials(specials)
    arr = _merges_to_arr(merges)
    n = ctypes.c_size_t(0)
    bo = ctypes.POINTER(ctypes.c_uint64)()
    try:
        if specials is not None:
            sp = _Specials(specials)
            p = L.bpe_decode_docs_special(ids.ctypes.data_as(ctypes.c_void_p), ids.size,
                                          off.ctypes.data_as(ctypes.c_void_p), off.size - 1, arr, sp.ref, int(device),
                                          ctypes.byref(n), ctypes.byref(bo))
        else:
            p = L.bpe_decode_docs(ids.ctypes.data_as(ctypes.c_void_p), ids.size, off.ctypes.data_as(ctypes.c_void_p),
                                  off.size - 1, arr, int(device), ctypes.byref(n), ctypes.byref(bo))
    finally:
        L.dyn_arr_free(arr)
    if not p:
        raise BpeError("bpe_decode_docs failed")
    raw = ctypes.string_at(p, n.value)
    b = [int(bo[d]) for d in range(off.size)]
    ctypes.CDLL(None).free(ctypes.c_void_p(p))
    ctypes.CDLL(None).free(ctypes.cast(bo, ctypes.c_void_p))
    return [raw[b[d]:b[d + 1]] for d in range(off.size - 1)]


def decompress(ids, merges):
    """Reference decompress (bpe.c:341): bytes of the ids, NUL bytes dropped."""
    L = _lib.load()
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    arr = _merges_to_arr(merges)
    try:
        p = L.decompress(ids.ctypes.data_as(_u32p), ids.size, arr)
    finally:
        L.dyn_arr_free(arr)
    if not p:
        raise BpeError("decompress failed")
    s = ctypes.string_at(p)
    ctypes.CDLL(None).free(ctypes.c_void_p(p))
    return s


def dump_pairs(path, merges):
    L = _lib.load()
    arr = _merges_to_arr(merges)
    try:
        ok = L.dump_pairs(os.fsencode(path), arr)
    finally:
        L.dyn_arr_free(arr)
    if not ok:
        raise BpeError("dump_pairs failed")


def read_pairs(path):
    L = _lib.load()
    arr = L.read_pairs(os.fsencode(path))
    if not arr:
        raise BpeError("read_pairs failed")
    try:
        return _arr_to_merges(arr)
    finally:
        L.dyn_arr_free(arr)


def _join_texts(texts):
    """(the texts joined as uint8, their byte offsets uint64[T + 1]); a str is encoded as UTF-8"""
    items = [t.encode("utf-8") if isinstance(t, str) else bytes(t) for t in texts]
    off = np.zeros(len(items) + 1, dtype=np.uint64)
    if items:
        off[1:] = np.cumsum(np.fromiter((len(t) for t in items), dtype=np.uint64, count=len(items)))
    return np.frombuffer(b"".join(items), dtype=np.uint8), off


def check_texts(text_off, n):
    """Raise BpeError unless text_off are the byte offsets of len(text_off) - 1 texts in n bytes: the first 0, rising,
    the last n, n plus a gap byte per text within the 2^32 - 2 positions of a context (bpe_ex.h bpe_texts_check).
    The message names the offending index.  No GPU."""
    off = np.ascontiguousarray(text_off, dtype=np.uint64).reshape(-1)
    if off.size < 1:
        raise BpeError("texts: offsets must hold len(texts) + 1 entries")
    msg = ctypes.create_string_buffer(400)
    if _lib.load().bpe_texts_check(off.ctypes.data_as(ctypes.c_void_p), off.size - 1, int(n), msg, len(msg)):
        raise BpeError(msg.value.decode(errors="replace"))
    return off


def texts_gap(data, text_off, lo=None, hi=None):
    """The bytes a context keeps of a text batch: every text followed by one gap byte 0x00 (bpe_ex.h bpe_texts_gap);
    with lo / hi the stretch [lo, hi) of them alone (bpe_texts_gap_range).  No GPU."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    off = check_texts(text_off, buf.size)
    total = buf.size + off.size - 1
    vp = ctypes.c_void_p
    if lo is None and hi is None:
        out = np.full(total, 0xAA, dtype=np.uint8)
        _lib.check(_lib.load().bpe_texts_gap(buf.ctypes.data_as(vp), buf.size, off.ctypes.data_as(vp), off.size - 1,
                                             out.ctypes.data_as(vp), out.size), "texts_gap")
        return out.tobytes()
    lo, hi = int(lo or 0), total if hi is None else int(hi)
    out = np.full(max(hi - lo, 0), 0xAA, dtype=np.uint8)
    _lib.check(_lib.load().bpe_texts_gap_range(buf.ctypes.data_as(vp), buf.size, off.ctypes.data_as(vp), off.size - 1,
                                               lo, hi, out.ctypes.data_as(vp)), "texts_gap")
    return out.tobytes()


SPAN_UNITS = {"byte": 0, "char": 1}  # bpe_gpu.h BPE_SPAN_BYTE, BPE_SPAN_CHAR


def _span_unit(unit, what):
    if unit not in SPAN_UNITS:
        raise BpeError(f"{what}: unit {unit!r} (have {sorted(SPAN_UNITS)})")
    return SPAN_UNITS[unit]


def _span_args(merges, specials, vocab):
    """(pairs pointer, merges, specials ref or None, vocabulary ref or None, the objects to keep) for the span calls"""
    m = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1)
    sp = check_specials(specials) if specials else None
    cv = vocab.c_vocab() if vocab is not None else None
    return (m.ctypes.data_as(ctypes.c_void_p) if m.size else None, m.size // 2, sp.ref if sp else None,
            cv.ref if cv else None, (m, sp, cv))


def span_lens(merges, specials=None, vocab=None):
    """The byte length of every token id (bpe_ex.h bpe_span_lens), uint32: a byte is 1 (NUL included), merge r the sum
    of its halves, special j len(specials[j]).  Indexed by internal id (256 + merges + specials entries) or, with
    vocab (a vocab.Vocab over the same merges and specials), by vocabulary id (vocab.size entries, a hole 0).  A
    merge that names an id at or above its own raises BpeError with its rank.  No GPU."""
    L = _lib.load()
    pairs, k, sp, cv, keep = _span_args(merges, specials, vocab)
    n = ctypes.c_size_t(0)
    msg = ctypes.create_string_buffer(400)
    rc = L.bpe_span_lens(pairs, k, sp, cv, None, 0, ctypes.byref(n), msg, len(msg))
    out = np.zeros(n.value if not rc else 0, dtype=np.uint32)
    if not rc:
        rc = L.bpe_span_lens(pairs, k, sp, cv, out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(n), msg, len(msg))
    if rc:
        raise BpeError(f"span_lens: {L.bpe_gpu_strerror(rc).decode()} ({msg.value.decode(errors='replace')})")
    return out


def token_spans_host(ids, text_off, data, byte_off, lens, unit="byte"):
    """The spans of ids held as texts, on the host in plain loops (bpe_ex.h bpe_token_spans_host: the definition
    Engine.token_spans is held to): text k has the ids [text_off[k], text_off[k + 1]) and the bytes
    [byte_off[k], byte_off[k + 1]) of data; lens is span_lens' table in the ids' numbering.  Returns uint32[n, 2],
    each span relative to its text's first byte, in bytes or (unit "char") characters.  An id outside the table and
    a text whose lengths do not sum to its bytes raise BpeError (the text's index in the message).  No GPU."""
    L = _lib.load()
    u = _span_unit(unit, "token_spans_host")
    ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
    toff, boff = _doc_offsets(text_off), _doc_offsets(byte_off)
    if toff.size < 1 or toff.size != boff.size:
        raise BpeError("token_spans_host: text_off and byte_off must both hold texts + 1 entries")
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    lens = np.ascontiguousarray(lens, dtype=np.uint32).reshape(-1)
    out = np.zeros((ids.size, 2), dtype=np.uint32)
    msg = ctypes.create_string_buffer(400)
    vp = ctypes.c_void_p
    rc = L.bpe_token_spans_host(ids.ctypes.data_as(vp) if ids.size else None, ids.size, toff.ctypes.data_as(vp),
                                toff.size - 1, buf.ctypes.data_as(vp) if buf.size else None, buf.size,
                                boff.ctypes.data_as(vp), lens.ctypes.data_as(vp) if lens.size else None, lens.size, u,
                                out.ctypes.data_as(vp) if ids.size else None, msg, len(msg))
    if rc:
        raise BpeError(f"token_spans_host: {L.bpe_gpu_strerror(rc).decode()} ({msg.value.decode(errors='replace')})")
    return out


def span_info():
    """{ids one thread of the span kernel takes per step, ids per workgroup step, ids per grid step, bytes per grid
    step of the character pass} (bpe_gpu_span_info; no GPU; for the tests)"""
    out = np.zeros(4, dtype=np.uint64)
    _lib.check(_lib.load().bpe_gpu_span_info(out.ctypes.data_as(ctypes.c_void_p)), "span_info")
    return {"per_thread": int(out[0]), "per_block": int(out[1]), "per_grid": int(out[2]), "lead_bytes_per_grid": int(out[3])}


STREAM_BOS, STREAM_EOS, STREAM_DROP_LAST = 1, 2, 4  # bpe_gpu.h BPE_STREAM_*
STREAM_NO_TEXT = 0xFFFFFFFF  # seg of a pad cell (BPE_STREAM_NO_TEXT)


def check_stream(seq_len, pad_id=0, bos_id=None, eos_id=None, drop_last=False, flags=None):
    """The description of a packed stream (bpe_gpu.h bpe_gpu_stream) that the packing calls take, checked by
    bpe_ex.h bpe_stream_check: seq_len in 1 .. 2^24, the ids any uint32 (None: no BOS / EOS).  flags (for the tests):
    the flag word as it is, in place of the one the arguments make.  Raises BpeError with the code's text and a
    message that names the field.  No GPU."""
    L = _lib.load()
    vals = [int(seq_len), int(pad_id), int(bos_id or 0), int(eos_id or 0)]
    f = (STREAM_BOS if bos_id is not None else 0) | (STREAM_EOS if eos_id is not None else 0) | \
        (STREAM_DROP_LAST if drop_last else 0) if flags is None else int(flags)
    if any(not 0 <= v <= 0xFFFFFFFF for v in vals + [f]):
        raise BpeError("stream: seq_len, pad_id, bos_id, eos_id and flags are uint32")
    s = _lib.Stream(vals[0], f, vals[2], vals[3], vals[1])
    msg = ctypes.create_string_buffer(400)
    rc = L.bpe_stream_check(ctypes.byref(s), msg, len(msg))
    if rc:
        raise BpeError(f"check_stream: {L.bpe_gpu_strerror(rc).decode()} ({msg.value.decode(errors='replace')})")
    return s


def pack_stream_host(ids, text_off, seq_len, pad_id, bos_id=None, eos_id=None, drop_last=False):
    """The training rows of ids held as texts, on the host in plain loops (bpe_ex.h bpe_pack_stream_host: the
    definition Engine.pack_stream is held to; the contract: bpe_gpu.h, "Packed streams"): every text wrapped in
    bos_id / eos_id (None: without), the texts joined end to end and cut into rows of seq_len ids, the last row
    filled with pad_id or, with drop_last, dropped unless full.  Returns (rows, seg, pos, N): uint32[R, seq_len]
    each, seg the text of every cell (0xFFFFFFFF in a pad cell), pos its position in that text's stretch of the row,
    N the cells of the stream.  No GPU."""
    L = _lib.load()
    s = check_stream(seq_len, pad_id, bos_id, eos_id, drop_last)
    ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
    toff = _doc_offsets(text_off)
    if toff.size < 1:
        raise BpeError("pack_stream_host: text_off must hold texts + 1 entries")
    vp = ctypes.c_void_p
    R, N = ctypes.c_size_t(0), ctypes.c_uint64(0)
    args = (ids.ctypes.data_as(vp) if ids.size else None, ids.size, toff.ctypes.data_as(vp), toff.size - 1, ctypes.byref(s))
    rc = L.bpe_pack_stream_host(*args, None, None, None, 0, ctypes.byref(R), ctypes.byref(N))
    if rc:  # (the description passed check_stream: what is left are the offsets)
        raise BpeError(f"pack_stream_host: {L.bpe_gpu_strerror(rc).decode()} (text_off must run from 0 to the number "
                       "of ids without falling)")
    rows, seg, pos = (np.zeros((R.value, s.seq_len), dtype=np.uint32) for _ in range(3))
    if R.value:
        _lib.check(L.bpe_pack_stream_host(*args, rows.ctypes.data_as(vp), seg.ctypes.data_as(vp), pos.ctypes.data_as(vp),
                                          R.value, ctypes.byref(R), ctypes.byref(N)), "pack_stream_host")
    return rows, seg, pos, int(N.value)


def stream_info():
    """{cells one lane of the four-cell packing kernel takes per step, cells per workgroup step, cells the largest grid
    takes in one step (past that many a workgroup takes several consecutive steps), texts a lane walks forward before
    it searches for itself} (bpe_gpu_stream_info; no GPU; for the tests)"""
    out = np.zeros(4, dtype=np.uint64)
    _lib.check(_lib.load().bpe_gpu_stream_info(out.ctypes.data_as(ctypes.c_void_p)), "stream_info")
    return {"per_thread": int(out[0]), "per_block": int(out[1]), "per_grid": int(out[2]), "walk": int(out[3])}


ROWS_PAD, ROWS_SKIP = 1, 2  # bpe_gpu.h BPE_ROWS_*


class _Rows:
    """a bpe_gpu.h bpe_gpu_rows and the skip array it points into"""

    def __init__(self, desc, skip):
        self.desc, self.skip, self.ref = desc, skip, ctypes.byref(desc)


def check_rows(pad_id=None, stop_ids=(), skip_ids=(), flags=None):
    """The description of an unpack (bpe_gpu.h bpe_gpu_rows) that unpack_rows_host and Engine.unpack_rows take,
    checked by bpe_ex.h bpe_rows_check: pad_id (None: rows are not padded), at most 8 stop_ids, at most 256 skip_ids
    (none, or None: nothing is skipped), every id a uint32.  flags (for the tests): the flag word as it is, in place of the one
    the arguments make.  Raises BpeError with the code's text and a message that names the field.  No GPU."""
    L = _lib.load()
    stops = [int(s) for s in stop_ids]
    skips = [] if skip_ids is None else [int(s) for s in np.asarray(skip_ids).reshape(-1).tolist()]
    pad = 0 if pad_id is None else int(pad_id)
    f = (ROWS_PAD if pad_id is not None else 0) | (ROWS_SKIP if skips else 0) if flags is None else int(flags)
    if any(not 0 <= v <= 0xFFFFFFFF for v in stops + skips + [pad, f]):
        raise BpeError("rows: pad_id, stop_ids, skip_ids and flags are uint32")
    skip = np.array(skips, dtype=np.uint32)
    d = _lib.Rows(f, pad, len(stops), (ctypes.c_uint32 * 8)(*stops[:8]), skip.size,
                  skip.ctypes.data_as(ctypes.c_void_p) if skip.size else None)
    msg = ctypes.create_string_buffer(400)
    rc = L.bpe_rows_check(ctypes.byref(d), msg, len(msg))
    if rc:
        raise BpeError(f"check_rows: {L.bpe_gpu_strerror(rc).decode()} ({msg.value.decode(errors='replace')})")
    return _Rows(d, skip)


ROWS_WHAT = ("a 2-D numpy array of uint32, int32, int64 or uint64 whose rows are contiguous, or a 2-D torch tensor of "
             "int32 or int64 on the engine's device with stride(1) == 1 and stride(0) >= shape[1]")


def _rows_numpy(rows, what):
    """(array, cell_bytes, B, L, row_stride in cells) of a numpy rows argument, without a copy where its rows are
    contiguous"""
    if rows.ndim != 2 or rows.dtype not in (np.uint32, np.int32, np.int64, np.uint64):
        raise BpeError(f"{what}: rows of shape {rows.shape} and dtype {rows.dtype}: pass {ROWS_WHAT}")
    B, L = rows.shape
    cb = rows.dtype.itemsize
    ok = (L <= 1 or rows.strides[1] == cb) and (B <= 1 or (rows.strides[0] % cb == 0 and rows.strides[0] >= L * cb
                                                           and rows.strides[0] > 0))
    if not ok or not rows.dtype.isnative:
        rows = np.ascontiguousarray(rows)
    stride = rows.strides[0] // cb if B > 1 else L
    return rows, cb, B, L, max(stride, L)


def _lens_numpy(lens, B, what):
    lens = np.ascontiguousarray(lens)
    if lens.shape != (B,) or lens.dtype.kind not in "iu" or (lens.size and (lens.min() < 0 or lens.max() > 0xFFFFFFFF)):
        raise BpeError(f"{what}: lens must hold one uint32 per row ({B})")
    return lens.astype(np.uint32)


def unpack_rows_host(rows, lens=None, pad_id=None, stop_ids=(), skip_ids=()):
    """The texts' ids of a grid of cells, on the host in plain loops (bpe_ex.h bpe_unpack_rows_host: the definition
    Engine.unpack_rows is held to; the contract: bpe_gpu.h, "Rows back to texts").  rows: a 2-D numpy array of uint32,
    int32, int64 or uint64; a 64-bit cell is an id only in 0 .. 2^32 - 1.  Row k's window is its first lens[k] cells
    (lens None: all); its text begins behind the leading cells equal to pad_id (None: at 0) and ends before the first
    cell that is one of stop_ids or pad_id, or at the window's end; ids in skip_ids are left out.  Returns (ids
    uint32[n], text_off uint64[B + 1], bounds uint32[B, 2]): row k's ids are ids[text_off[k]:text_off[k + 1]] and
    bounds[k] = (start, end).  No GPU."""
    L_ = _lib.load()
    d = check_rows(pad_id, stop_ids, skip_ids)
    rows, cb, B, L, stride = _rows_numpy(np.asarray(rows), "unpack_rows_host")
    vp = ctypes.c_void_p
    if lens is not None:
        lens = _lens_numpy(lens, B, "unpack_rows_host")
    n = ctypes.c_size_t(0)
    msg = ctypes.create_string_buffer(400)
    args = (rows.ctypes.data_as(vp) if rows.size else None, cb, B, L, stride,
            lens.ctypes.data_as(vp) if lens is not None and B else None, d.ref)

    rc = L_.bpe_unpack_rows_host(*args, None, 0, ctypes.byref(n), None, None, msg, len(msg))
    if rc:
        raise BpeError(f"unpack_rows_host: {L_.bpe_gpu_strerror(rc).decode()} ({msg.value.decode(errors='replace')})")
    ids = np.zeros(n.value, dtype=np.uint32)
    text_off = np.zeros(B + 1, dtype=np.uint64)
    bounds = np.zeros((B, 2), dtype=np.uint32)
    rc = L_.bpe_unpack_rows_host(*args, ids.ctypes.data_as(vp), ids.size, ctypes.byref(n), text_off.ctypes.data_as(vp),
                                 bounds.ctypes.data_as(vp), msg, len(msg))
    if rc:
        raise BpeError(f"unpack_rows_host: {L_.bpe_gpu_strerror(rc).decode()} ({msg.value.decode(errors='replace')})")
    return ids, text_off, bounds


def rows_info():
    """{cells one lane of the vector unpacking kernels takes per step, cells a wave (which owns a row) takes per step
    then, rows per workgroup, rows the largest grid takes in one step} (bpe_gpu_rows_info; the one-cell variants take a
    quarter of the first two; no GPU; for the tests)"""
    out = np.zeros(4, dtype=np.uint64)
    _lib.check(_lib.load().bpe_gpu_rows_info(out.ctypes.data_as(ctypes.c_void_p)), "rows_info")
    return {"per_lane": int(out[0]), "per_wave": int(out[1]), "rows_per_block": int(out[2]), "rows_per_grid": int(out[3])}


PACK_SIDES = {"right": 0, "left": 1}  # the side a longer text is cut at: "right" keeps its first ids, "left" its last


class Engine:
    """Direct handle on one GPU context (bpe_gpu.h) -- used by bench.py to keep
    the corpus resident in HBM and time the training loop alone."""

    def __init__(self, device=0):
        self.L = _lib.load()
        self.ctx = ctypes.c_void_p()
        _lib.check(self.L.bpe_gpu_create(int(device), ctypes.byref(self.ctx)), "bpe_gpu_create")

    def close(self):
        if self.ctx:
            self.L.bpe_gpu_destroy(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load(self, data: bytes):
        buf = np.frombuffer(data, dtype=np.uint8)
        _lib.check(self.L.bpe_gpu_load(self.ctx, buf.ctypes.data_as(ctypes.c_void_p), buf.size), "load")

    def load_texts(self, texts, offsets=None):
        """load a batch of texts (bytes-like objects; a str is encoded as UTF-8), each to be split and encoded on
        its own (bpe_gpu_load_texts): split() and encode_split() then honour the breaks between them, ids(),
        doc_offsets() and split_offsets() describe the texts joined with nothing between them, and
        text_offsets() / pack_texts() give the ids per text.  Any other load ends the batch.  With offsets
        (uint64, texts + 1 entries) `texts` is the texts' bytes already joined.  Returns the number of texts."""
        if offsets is None:
            buf, off = _join_texts(texts)
        else:
            buf, off = np.frombuffer(texts, dtype=np.uint8), _doc_offsets(offsets)
            if off.size < 1:
                raise BpeError("load_texts: offsets must hold len(texts) + 1 entries")
        vp = ctypes.c_void_p
        _lib.check(self.L.bpe_gpu_load_texts(self.ctx, buf.ctypes.data_as(vp), buf.size, off.ctypes.data_as(vp),
                                             off.size - 1), "load_texts")
        return off.size - 1

    def text_offsets(self):
        """id offsets of the texts after encode_split() over a text batch (uint64, texts + 1 entries:
        text k's ids are ids()[text_offsets()[k]:text_offsets()[k + 1]]; bpe_gpu_fetch_text_offsets)"""
        n = ctypes.c_size_t(0)
        _lib.check(self.L.bpe_gpu_fetch_text_offsets(self.ctx, None, 0, ctypes.byref(n)), "fetch_text_offsets")
        out = np.zeros(n.value, dtype=np.uint64)
        _lib.check(self.L.bpe_gpu_fetch_text_offsets(self.ctx, out.ctypes.data_as(ctypes.c_void_p), n.value,
                                                     ctypes.byref(n)), "fetch_text_offsets")
        return out

    def pack_texts(self, row_len, pad_id, side="right", out=None):
        """the resident ids of a text batch (mapped or not) as rows (bpe_gpu_pack_texts): (rows uint32[texts, row_len],
        lens uint32[texts]) with lens[k] = min(ids of text k, row_len); a longer text is cut at `side` ("right": its
        first row_len ids stay, "left": its last), pad_id (any uint32) fills the row behind the ids.  Returns numpy
        arrays.  out: a contiguous torch tensor of 32-bit integers, [texts, row_len], on this engine's device: the
        rows are written into it on the device, no id passes through the host, and (out, lens), lens a torch int32
        tensor beside it, is returned."""
        if side not in PACK_SIDES:
            raise BpeError(f"pack_texts: side {side!r} (have {sorted(PACK_SIDES)})")
        row_len, pad_id = int(row_len), int(pad_id)
        if not 0 <= pad_id <= 0xFFFFFFFF or not 0 <= row_len <= 0xFFFFFFFF:
            raise BpeError("pack_texts: row_len and pad_id are uint32")
        T = self.text_offsets().size - 1
        vp = ctypes.c_void_p
        if out is None:
            rows = np.zeros((T, row_len), dtype=np.uint32)
            lens = np.zeros(T, dtype=np.uint32)
            _lib.check(self.L.bpe_gpu_pack_texts(self.ctx, row_len, pad_id, PACK_SIDES[side],
                                                 rows.ctypes.data_as(vp) if rows.size else None, 0,
                                                 lens.ctypes.data_as(vp) if T else None), "pack_texts")
            return rows, lens
        import torch
        if (not isinstance(out, torch.Tensor) or not out.is_cuda or out.element_size() != 4 or out.is_floating_point()
                or tuple(out.shape) != (T, row_len) or not out.is_contiguous()):
            raise BpeError(f"pack_texts: out must be a contiguous 32-bit integer tensor of shape ({T}, {row_len}) on the GPU")
        lens = torch.empty(T, dtype=torch.int32, device=out.device)
        torch.cuda.current_stream(out.device).synchronize()  # (the call writes on the context's stream)
        _lib.check(self.L.bpe_gpu_pack_texts(self.ctx, row_len, pad_id, PACK_SIDES[side],
                                             vp(out.data_ptr()) if out.numel() else None, 1,
                                             vp(lens.data_ptr()) if T else None), "pack_texts")
        return out, lens

    def token_spans(self, merges, specials=None, vocab=None, unit="byte"):
        """the span of every resident id of the last encode_split() / encode_docs() in its text, uint32[n, 2]
        (bpe_gpu_token_spans, computed and kept on the device): in bytes, or with unit "char" in characters as
        `tokenizers`' Encoding.offsets counts them (bpe_gpu.h, "Token spans").  In a text batch every span is
        relative to its own text.  merges / specials: those of the encode and the split; vocab: needed after
        map_ids(), refused before it.  A list that is not the encode's raises BpeError (BPE_GPU_EINVAL for another
        count, BPE_GPU_EDATA when the lengths do not sum to the text) and the engine goes on."""
        u = _span_unit(unit, "token_spans")
        pairs, k, sp, cv, keep = _span_args(merges, specials, vocab)
        _lib.check(self.L.bpe_gpu_token_spans(self.ctx, pairs, k, sp, cv, u), "token_spans")
        n = ctypes.c_size_t(0)
        _lib.check(self.L.bpe_gpu_fetch_token_spans(self.ctx, None, 0, ctypes.byref(n)), "fetch_token_spans")
        out = np.zeros((n.value, 2), dtype=np.uint32)
        if n.value:
            _lib.check(self.L.bpe_gpu_fetch_token_spans(self.ctx, out.ctypes.data_as(ctypes.c_void_p), n.value,
                                                        ctypes.byref(n)), "fetch_token_spans")
        return out

    def pack_spans(self, row_len, side="right", out=None):
        """the spans of the last token_spans() over a text batch as rows, uint32[texts, row_len, 2]
        (bpe_gpu_pack_spans): cut as pack_texts(row_len, ., side) cuts the ids, the cells behind the ids (0, 0); with
        side "left" the spans stay relative to the whole text.  out: a contiguous torch tensor of 32-bit integers,
        [texts, row_len, 2], on this engine's device: written on the device and returned."""
        if side not in PACK_SIDES:
            raise BpeError(f"pack_spans: side {side!r} (have {sorted(PACK_SIDES)})")
        row_len = int(row_len)
        if not 0 <= row_len <= 0xFFFFFFFF:
            raise BpeError("pack_spans: row_len is a uint32")
        T = self.text_offsets().size - 1
        vp = ctypes.c_void_p
        if out is None:
            rows = np.zeros((T, row_len, 2), dtype=np.uint32)
            _lib.check(self.L.bpe_gpu_pack_spans(self.ctx, row_len, PACK_SIDES[side],
                                                 rows.ctypes.data_as(vp) if rows.size else None, 0), "pack_spans")
            return rows
        import torch
        if (not isinstance(out, torch.Tensor) or not out.is_cuda or out.element_size() != 4 or out.is_floating_point()
                or tuple(out.shape) != (T, row_len, 2) or not out.is_contiguous()):
            raise BpeError(f"pack_spans: out must be a contiguous 32-bit integer tensor of shape ({T}, {row_len}, 2) on the GPU")
        torch.cuda.current_stream(out.device).synchronize()  # (the call writes on the context's stream)
        _lib.check(self.L.bpe_gpu_pack_spans(self.ctx, row_len, PACK_SIDES[side],
                                             vp(out.data_ptr()) if out.numel() else None, 1), "pack_spans")
        return out

    def stream_rows(self, seq_len, bos_id=None, eos_id=None, drop_last=False):
        """(R, N) of pack_stream() with these arguments: the rows, and the cells of the stream (the query of
        bpe_gpu_pack_stream; nothing is launched)"""
        s = check_stream(seq_len, 0, bos_id, eos_id, drop_last)
        R, N = ctypes.c_size_t(0), ctypes.c_uint64(0)
        _lib.check(self.L.bpe_gpu_pack_stream(self.ctx, ctypes.byref(s), None, None, None, 0, 0, ctypes.byref(R),
                                              ctypes.byref(N)), "pack_stream")
        return int(R.value), int(N.value)

    def pack_stream(self, seq_len, pad_id, bos_id=None, eos_id=None, drop_last=False, segments=False, positions=False,
                    out=None):
        """the resident ids of a text batch (mapped or not) as training rows (bpe_gpu_pack_stream; the contract:
        bpe_gpu.h, "Packed streams"): every text wrapped in bos_id / eos_id (any uint32; None: without), the texts
        joined end to end and cut into rows of exactly seq_len ids; nothing is truncated, the last row is filled with
        pad_id or, with drop_last, dropped unless full.  Returns numpy uint32[R, seq_len] arrays: rows, then with
        segments seg (the index of every cell's text in the batch, 0xFFFFFFFF in a pad cell: a block-diagonal
        attention mask is seg[r, i] == seg[r, j]) and with positions pos (the cell's position in its text's stretch
        of the row, 0 in a pad cell: position ids); rows alone when neither is asked for.  out=(rows, seg or None,
        pos or None): contiguous torch tensors of 32-bit integers, [R, seq_len] (R of stream_rows()), on this
        engine's device: written on the device, no id passes through the host, and the tuple is returned."""
        s = check_stream(seq_len, pad_id, bos_id, eos_id, drop_last)
        R, N = self.stream_rows(seq_len, bos_id, eos_id, drop_last)
        vp = ctypes.c_void_p
        if out is None:
            arrs = [np.zeros((R, s.seq_len), dtype=np.uint32) for _ in range(1 + bool(segments) + bool(positions))]
            ptrs = [a.ctypes.data_as(vp) if a.size else None for a in arrs]
            seg = ptrs[1] if segments else None
            pos = ptrs[-1] if positions else None
            if R:
                _lib.check(self.L.bpe_gpu_pack_stream(self.ctx, ctypes.byref(s), ptrs[0], seg, pos, 0, R, None, None),
                           "pack_stream")
            return tuple(arrs) if len(arrs) > 1 else arrs[0]
        import torch
        if not isinstance(out, (tuple, list)) or len(out) != 3 or out[0] is None:
            raise BpeError("pack_stream: out must be (rows, seg or None, pos or None)")
        for t in out:
            if t is None:
                continue
            if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.element_size() != 4 or t.is_floating_point()
                    or tuple(t.shape) != (R, s.seq_len) or not t.is_contiguous()):
                raise BpeError(f"pack_stream: out must hold contiguous 32-bit integer tensors of shape ({R}, {s.seq_len}) "
                               "on the GPU")
            if t.device != out[0].device:
                raise BpeError("pack_stream: the tensors of out lie on different devices")
        torch.cuda.current_stream(out[0].device).synchronize()  # (the call writes on the context's stream)
        ptrs = [vp(t.data_ptr()) if t is not None and t.numel() else None for t in out]
        if R:
            _lib.check(self.L.bpe_gpu_pack_stream(self.ctx, ctypes.byref(s), ptrs[0], ptrs[1], ptrs[2], 1, R, None, None),
                       "pack_stream")
        return tuple(out)

    def unpack_rows(self, rows, lens=None, pad_id=None, stop_ids=(), skip_ids=()):
        """the texts' ids of a grid of cells, cut on the device (bpe_gpu_unpack_rows; the contract: bpe_gpu.h, "Rows
        back to texts"; the arguments: unpack_rows_host).  rows: a numpy array as unpack_rows_host takes it, or a 2-D
        torch tensor of int32 or int64 on this engine's device with stride(1) == 1 and stride(0) >= shape[1] (so
        out[:, P:] of a contiguous tensor is read where it lies, without a copy): no id passes through the host.
        lens: a numpy array or a torch int32 tensor on the same device.  The ids, their offsets and the bounds stay on
        the device for decode_rows() and are returned as numpy arrays (ids uint32[n], text_off uint64[B + 1], bounds
        uint32[B, 2]).  They live apart from the resident ids of an encode: neither disturbs the other."""
        self._unpack_rows(rows, lens, pad_id, stop_ids, skip_ids)
        return self.fetch_rows()

    def _unpack_rows(self, rows, lens, pad_id, stop_ids, skip_ids):
        d = check_rows(pad_id, stop_ids, skip_ids)
        vp = ctypes.c_void_p
        n = ctypes.c_size_t(0)
        if isinstance(rows, np.ndarray) or not hasattr(rows, "data_ptr"):
            rows, cb, B, L, stride = _rows_numpy(np.asarray(rows), "unpack_rows")
            rp, on_dev = (rows.ctypes.data_as(vp) if rows.size else None), 0
            dev = None
        else:
            import torch
            if (not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.dtype not in (torch.int32, torch.int64)
                    or not rows.is_cuda or (rows.shape[1] > 1 and rows.stride(1) != 1)
                    or (rows.shape[0] > 1 and rows.stride(0) < rows.shape[1])):
                where = f" on {rows.device}" if isinstance(rows, torch.Tensor) else ""
                raise BpeError(f"unpack_rows: rows of shape {tuple(rows.shape)}, dtype {rows.dtype} and strides "
                               f"{tuple(rows.stride())}{where}: pass {ROWS_WHAT}")
            (B, L), cb, dev = rows.shape, rows.element_size(), rows.device
            stride = max(rows.stride(0), L) if B > 1 else L
            rp, on_dev = (vp(rows.data_ptr()) if rows.numel() else None), 1
            torch.cuda.current_stream(dev).synchronize()  # (the call reads on the context's stream)
        lp, lens_dev = None, 0
        if lens is not None and hasattr(lens, "data_ptr"):
            import torch
            if (not isinstance(lens, torch.Tensor) or lens.dtype != torch.int32 or tuple(lens.shape) != (B,)
                    or not lens.is_contiguous() or not lens.is_cuda or (dev is not None and lens.device != dev)):
                raise BpeError(f"unpack_rows: lens must be a numpy array or a contiguous torch int32 tensor of shape ({B},) "
                               "on the device of rows")
            if dev is None:
                torch.cuda.current_stream(lens.device).synchronize()
            lp, lens_dev = (vp(lens.data_ptr()) if B else None), 1
        elif lens is not None:
            lens = _lens_numpy(lens, B, "unpack_rows")
            lp = lens.ctypes.data_as(vp) if B else None
        _lib.check(self.L.bpe_gpu_unpack_rows(self.ctx, rp, on_dev, cb, B, L, stride, lp, lens_dev, d.ref, ctypes.byref(n)),
                   "unpack_rows")
        return B, n.value

    def fetch_rows(self):
        """(ids, text_off, bounds) of the last unpack_rows(), as it returned them (bpe_gpu_fetch_rows)"""
        n, B = ctypes.c_size_t(0), ctypes.c_size_t(0)
        _lib.check(self.L.bpe_gpu_fetch_rows(self.ctx, None, 0, ctypes.byref(n), None, None, 0, ctypes.byref(B)), "fetch_rows")
        ids = np.zeros(n.value, dtype=np.uint32)
        text_off = np.zeros(B.value + 1, dtype=np.uint64)
        bounds = np.zeros((B.value, 2), dtype=np.uint32)
        vp = ctypes.c_void_p
        _lib.check(self.L.bpe_gpu_fetch_rows(self.ctx, ids.ctypes.data_as(vp) if n.value else None, n.value, ctypes.byref(n),
                                             text_off.ctypes.data_as(vp), bounds.ctypes.data_as(vp) if B.value else None,
                                             B.value, ctypes.byref(B)), "fetch_rows")
        return ids, text_off, bounds

    def decode_rows(self, merges, specials=None, vocab=None):
        """(bytes, byte offsets) of the last unpack_rows(), row k's text being bytes[off[k]:off[k + 1]]
        (bpe_gpu_decode_rows): what decode_docs(ids, text_off, merges, specials, vocab) of the unpacked ids gives,
        without the ids leaving the device.  The unpacked ids stay and can be decoded again."""
        m = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1)
        vp = ctypes.c_void_p
        sp = cv = None
        if specials is not None:
            check_specials(specials)
            sp = _Specials(specials)
        if vocab is not None:
            cv = vocab.c_vocab()
        B, n = ctypes.c_size_t(0), ctypes.c_size_t(0)
        args = (self.ctx, m.ctypes.data_as(vp), m.size // 2, sp.ref if sp else None, cv.ref if cv else None)
        _lib.check(self.L.bpe_gpu_decode_rows(*args, None, 0, ctypes.byref(n), None), "decode_rows")
        _lib.check(self.L.bpe_gpu_fetch_rows(self.ctx, None, 0, None, None, None, 0, ctypes.byref(B)), "fetch_rows")
        out = np.zeros(max(n.value, 1), dtype=np.uint8)
        bo = np.zeros(B.value + 1, dtype=np.uint64)
        _lib.check(self.L.bpe_gpu_decode_rows(*args, out.ctypes.data_as(vp), out.size, ctypes.byref(n), bo.ctypes.data_as(vp)),
                   "decode_rows")
        return out[: n.value].tobytes(), bo

    def load_file(self, path):
        """stream a file into HBM (bpe_gpu_load_fd: pinned double-buffered
        staging, the corpus ends at the first NUL); returns the bytes loaded"""
        fd = os.open(path, os.O_RDONLY)
        try:
            n = ctypes.c_size_t(0)
            _lib.check(self.L.bpe_gpu_load_fd(self.ctx, fd, os.fstat(fd).st_size, ctypes.byref(n)), "load_fd")
        finally:
            os.close(fd)
        return n.value

    def synth(self, seed, n, offset=0):
        _lib.check(self.L.bpe_gpu_synth(self.ctx, int(seed), int(n), int(offset)), "synth")

    def train(self, max_merges=-1, fast=False):
        """fast=True: schedule-free tie rule everywhere (bpe_gpu.h BPE_GPU_FAST)"""
        k = ctypes.c_size_t(0)
        _lib.check(self.L.bpe_gpu_train_ex(self.ctx, int(max_merges), 1 if fast else 0, ctypes.byref(k)), "train")
        return k.value

    def encode(self, merges):
        m = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1)
        _lib.check(self.L.bpe_gpu_encode(self.ctx, m.ctypes.data_as(ctypes.c_void_p), m.size // 2), "encode")

    def encode_docs(self, offsets, merges):
        """encode the resident bytes as documents: document d is bytes
        [offsets[d], offsets[d + 1]) (bpe_gpu_encode_docs); then ids(), doc_offsets(), docs_info()"""
        off = _doc_offsets(offsets)
        if off.size < 1:
            raise BpeError("encode_docs: offsets must hold ndocs + 1 entries")
        m = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1)
        _lib.check(self.L.bpe_gpu_encode_docs(self.ctx, off.ctypes.data_as(ctypes.c_void_p), off.size - 1,
                                              m.ctypes.data_as(ctypes.c_void_p), m.size // 2), "encode_docs")

    def split(self, rule="words", specials=None):
        """split the resident bytes into pieces on the device (rule: a preset
        name, "lines", "words", "gpt2", "gpt2_unicode" or "cl100k", or a (cls, brk) pair, see split_rule); the offsets stay in HBM for
        encode_split().  With specials (a list of bytes-like objects, see check_specials) every occurrence of
        one is a piece of its own (bpe_gpu_split_special); they last as long as the offsets, and a split
        without them forgets them.  Returns the number of pieces."""
        nd = ctypes.c_size_t(0)
        if specials is not None:
            check_specials(specials)  # (before any launch)
            sp = _Specials(specials)
            preset, pc, pb, keep = _rule_args(rule)
            _lib.check(self.L.bpe_gpu_split_special(self.ctx, preset, pc, pb, sp.ref, ctypes.byref(nd)), "split")
            return nd.value
        if _no_tables(rule):  # the preset call (bpe_gpu_split_preset)
            _lib.check(self.L.bpe_gpu_split_preset(self.ctx, SPLIT_PRESETS[rule], ctypes.byref(nd)), "split")
            return nd.value
        cls, brk = _rule_tables(rule)
        _lib.check(self.L.bpe_gpu_split(self.ctx, cls.ctypes.data_as(ctypes.c_void_p),
                                        brk.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nd)), "split")
        return nd.value

    def split_offsets(self):
        """byte offsets of the last split (uint64: the piece starts followed by n)"""
        n = ctypes.c_size_t(0)
        _lib.check(self.L.bpe_gpu_fetch_split_offsets(self.ctx, None, 0, ctypes.byref(n)), "fetch_split_offsets")
        out = np.zeros(n.value, dtype=np.uint64)
        _lib.check(self.L.bpe_gpu_fetch_split_offsets(self.ctx, out.ctypes.data_as(ctypes.c_void_p), n.value,
                                                      ctypes.byref(n)), "fetch_split_offsets")
        return out

    SPLIT_SPECIAL_INFO = ("specials", "matches", "find_passes", "match_capacity")

    def split_special_info(self):
        """counters of the last split's specials (bpe_gpu_split_special_info; zeros after a split without)"""
        out = np.zeros(4, dtype=np.uint64)
        _lib.check(self.L.bpe_gpu_split_special_info(self.ctx, out.ctypes.data_as(ctypes.c_void_p)), "split_special_info")
        return {k: int(out[i]) for i, k in enumerate(self.SPLIT_SPECIAL_INFO)}

    def special_pieces(self):
        """the special pieces of the last split in order: (piece index uint64, index of its special uint32)"""
        n = ctypes.c_size_t(0)
        _lib.check(self.L.bpe_gpu_fetch_special_pieces(self.ctx, None, None, 0, ctypes.byref(n)), "fetch_special_pieces")
        piece = np.zeros(max(n.value, 1), dtype=np.uint64)
        index = np.zeros(max(n.value, 1), dtype=np.uint32)
        vp = ctypes.c_void_p
        _lib.check(self.L.bpe_gpu_fetch_special_pieces(self.ctx, piece.ctypes.data_as(vp), index.ctypes.data_as(vp),
                                                       n.value, ctypes.byref(n)), "fetch_special_pieces")
        return piece[: n.value], index[: n.value]

    def encode_split(self, merges):
        """encode_docs over the last split's resident offsets (bpe_gpu_encode_split);
        then ids(), doc_offsets(), docs_info() as after encode_docs.  After a split with specials
        every special piece holds the one id 256 + len(merges) + j."""
        m = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1)
        _lib.check(self.L.bpe_gpu_encode_split(self.ctx, m.ctypes.data_as(ctypes.c_void_p), m.size // 2), "encode_split")

    def train_split(self, max_merges=-1):
        """train on the pieces of the last split (bpe_gpu_train_split): the bytes, the
        offsets and earlier ids stay; then split_merges(), train_split_info(), piece_table().
        Returns the number of merges."""
        k = ctypes.c_size_t(0)
        _lib.check(self.L.bpe_gpu_train_split(self.ctx, int(max_merges), ctypes.byref(k)), "train_split")
        return k.value

    def split_merges(self):
        """the merges of the last train_split, (k, 2) uint32"""
        cnt = ctypes.c_size_t(0)
        _lib.check(self.L.bpe_gpu_fetch_split_merges(self.ctx, None, 0, ctypes.byref(cnt)), "fetch_split_merges")
        out = np.zeros(2 * max(cnt.value, 1), dtype=np.uint32)
        _lib.check(self.L.bpe_gpu_fetch_split_merges(self.ctx, out.ctypes.data_as(ctypes.c_void_p), cnt.value,
                                                     ctypes.byref(cnt)), "fetch_split_merges")
        return out[: 2 * cnt.value].reshape(-1, 2)

    TRAIN_SPLIT_INFO = ("pieces", "entries", "entry_bytes", "long_pieces", "merges", "stop_reason", "dedup_max",
                        "table_slots")

    def train_split_info(self):
        """counters of the last train_split (bpe_gpu_train_split_info)"""
        out = np.zeros(8, dtype=np.uint64)
        _lib.check(self.L.bpe_gpu_train_split_info(self.ctx, out.ctypes.data_as(ctypes.c_void_p)), "train_split_info")
        return {k: int(out[i]) for i, k in enumerate(self.TRAIN_SPLIT_INFO)}

    def piece_table(self):
        """the distinct pieces of the last train_split in start order: (start uint64,
        length uint32, count uint32); a piece longer than dedup_max is an entry of its own"""
        n = ctypes.c_size_t(0)
        _lib.check(self.L.bpe_gpu_fetch_piece_table(self.ctx, None, None, None, 0, ctypes.byref(n)), "fetch_piece_table")
        st = np.zeros(max(n.value, 1), dtype=np.uint64)
        ln = np.zeros(max(n.value, 1), dtype=np.uint32)
        ct = np.zeros(max(n.value, 1), dtype=np.uint32)
        vp = ctypes.c_void_p
        _lib.check(self.L.bpe_gpu_fetch_piece_table(self.ctx, st.ctypes.data_as(vp), ln.ctypes.data_as(vp),
                                                    ct.ctypes.data_as(vp), n.value, ctypes.byref(n)), "fetch_piece_table")
        return st[: n.value], ln[: n.value], ct[: n.value]

    def doc_offsets(self):
        """id offsets of the last encode_docs (uint64, ndocs + 1 entries)"""
        n = ctypes.c_size_t(0)
        _lib.check(self.L.bpe_gpu_fetch_doc_offsets(self.ctx, None, 0, ctypes.byref(n)), "fetch_doc_offsets")
        out = np.zeros(n.value, dtype=np.uint64)
        _lib.check(self.L.bpe_gpu_fetch_doc_offsets(self.ctx, out.ctypes.data_as(ctypes.c_void_p), n.value,
                                                    ctypes.byref(n)), "fetch_doc_offsets")
        return out

    DOCS_INFO = ("ndocs", "docs_fallback", "windows", "windows_failed", "core", "halo")

    def docs_info(self):
        """counters of the last encode_docs (bpe_gpu_docs_info)"""
        out = np.zeros(8, dtype=np.uint64)
        _lib.check(self.L.bpe_gpu_docs_info(self.ctx, out.ctypes.data_as(ctypes.c_void_p)), "docs_info")
        return {k: int(out[i]) for i, k in enumerate(self.DOCS_INFO)}

    def map_ids(self, vocab):
        """rewrite the resident ids of the last encode in place to the ids of vocab (a vocab.Vocab):
        ids(), ids_checksum() and doc_offsets() serve them afterwards, the offsets unchanged
        (bpe_gpu_map_ids).  A second map_ids, or one without ids, raises BpeError (BPE_GPU_ESTATE)."""
        _lib.check(self.L.bpe_gpu_map_ids(self.ctx, vocab.c_vocab().ref), "map_ids")

    def decode_docs(self, ids, offsets, merges, specials=None, vocab=None):
        """(bytes, byte offsets) of ids held as documents (bpe_gpu_decode_docs); with specials (see split) the
        id 256 + len(merges) + j is specials[j] (bpe_gpu_decode_docs_special); with vocab (a vocab.Vocab
        over the same merges and specials) the ids are the vocabulary's (bpe_gpu_decode_docs_vocab)"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        off = _doc_offsets(offsets)
        if off.size < 1:
            raise BpeError("decode_docs: offsets must hold ndocs + 1 entries")
        m = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1)
        n = ctypes.c_size_t(0)
        vp = ctypes.c_void_p
        args = (self.ctx, ids.ctypes.data_as(vp), ids.size, off.ctypes.data_as(vp), off.size - 1, m.ctypes.data_as(vp),
                m.size // 2)
        fn = self.L.bpe_gpu_decode_docs
        if specials is not None:
            check_specials(specials)
            sp = _Specials(specials)
            fn, args = self.L.bpe_gpu_decode_docs_special, args + (sp.ref,)
        if vocab is not None:
            cv = vocab.c_vocab()
            fn = self.L.bpe_gpu_decode_docs_vocab
            args = (args if specials is not None else args + (None,)) + (cv.ref,)
        _lib.check(fn(*args, None, 0, ctypes.byref(n), None), "decode_docs")
        out = np.zeros(max(n.value, 1), dtype=np.uint8)
        bo = np.zeros(off.size, dtype=np.uint64)
        _lib.check(fn(*args, out.ctypes.data_as(vp), out.size, ctypes.byref(n), bo.ctypes.data_as(vp)), "decode_docs")
        return out[: n.value].tobytes(), bo

    def merges(self):
        cnt = ctypes.c_size_t(0)
        _lib.check(self.L.bpe_gpu_fetch_merges(self.ctx, None, 0, ctypes.byref(cnt)), "fetch_merges")
        out = np.zeros(2 * max(cnt.value, 1), dtype=np.uint32)
        _lib.check(self.L.bpe_gpu_fetch_merges(self.ctx, out.ctypes.data_as(ctypes.c_void_p), cnt.value,
                                               ctypes.byref(cnt)), "fetch_merges")
        return out[: 2 * cnt.value].reshape(-1, 2)

    def ids(self):
        n = ctypes.c_size_t(0)
        _lib.check(self.L.bpe_gpu_fetch_ids(self.ctx, None, 0, ctypes.byref(n)), "fetch_ids")
        out = np.zeros(max(n.value, 1), dtype=np.uint32)
        _lib.check(self.L.bpe_gpu_fetch_ids(self.ctx, out.ctypes.data_as(ctypes.c_void_p), n.value,
                                            ctypes.byref(n)), "fetch_ids")
        return out[: n.value]

    def decode(self, ids, merges):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        m = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1)
        n = ctypes.c_size_t(0)
        vp = ctypes.c_void_p
        _lib.check(self.L.bpe_gpu_decode(self.ctx, ids.ctypes.data_as(vp), ids.size, m.ctypes.data_as(vp),
                                         m.size // 2, None, 0, ctypes.byref(n)), "decode")
        out = np.zeros(max(n.value, 1), dtype=np.uint8)
        _lib.check(self.L.bpe_gpu_decode(self.ctx, ids.ctypes.data_as(vp), ids.size, m.ctypes.data_as(vp),
                                         m.size // 2, out.ctypes.data_as(vp), out.size, ctypes.byref(n)),
                   "decode")
        return out[: n.value].tobytes()

    def stats(self):
        st = GpuStats()
        _lib.check(self.L.bpe_gpu_get_stats(self.ctx, ctypes.byref(st)), "stats")
        return st.as_dict()

    def set_merge_log(self, on=True):
        """per-merge records for the next trainings (bpe_gpu_set_merge_log)"""
        _lib.check(self.L.bpe_gpu_set_merge_log(self.ctx, 1 if on else 0), "set_merge_log")

    def merge_log(self):
        """the last training's per-merge records (count, ties, batch, batch_pos,
        distinct_pairs, tokens, t_us) as a numpy structured array"""
        n = ctypes.c_size_t(0)
        _lib.check(self.L.bpe_gpu_fetch_merge_log(self.ctx, None, 0, ctypes.byref(n)), "fetch_merge_log")
        recs = (_lib.MergeRec * max(n.value, 1))()
        _lib.check(self.L.bpe_gpu_fetch_merge_log(self.ctx, recs, n.value, ctypes.byref(n)), "fetch_merge_log")
        dt = np.dtype([(f, np.uint32 if t is ctypes.c_uint32 else np.uint64 if t is ctypes.c_uint64 else np.float64)
                       for f, t in _lib.MergeRec._fields_])
        return np.frombuffer(bytes(recs), dtype=dt, count=n.value).copy()

    def ids_checksum(self, base=0):
        """position-keyed checksum of the ids in HBM (bpe_gpu_ids_checksum)"""
        s = ctypes.c_uint64()
        _lib.check(self.L.bpe_gpu_ids_checksum(self.ctx, int(base), ctypes.byref(s)), "ids_checksum")
        return s.value

    EVENT_KINDS = {1: "relist", 2: "hot_rebuild", 3: "table_grow", 4: "mode"}

    def events(self):
        """run events of the last training (bpe_gpu_fetch_events): a list of
        (kind, merges committed before it), kind in EVENT_KINDS' values"""
        n = ctypes.c_size_t(0)
        _lib.check(self.L.bpe_gpu_fetch_events(self.ctx, None, 0, ctypes.byref(n)), "fetch_events")
        buf = (ctypes.c_uint64 * max(n.value, 1))()
        _lib.check(self.L.bpe_gpu_fetch_events(self.ctx, buf, n.value, ctypes.byref(n)), "fetch_events")
        return [(self.EVENT_KINDS.get(buf[i] >> 56, str(buf[i] >> 56)), buf[i] & ((1 << 56) - 1))
                for i in range(n.value)]

    def trim(self):
        """give the context's device memory back (bpe_gpu_trim); load again before use"""
        _lib.check(self.L.bpe_gpu_trim(self.ctx), "trim")

    def set_profile(self, on=True):
        _lib.check(self.L.bpe_gpu_set_profile(self.ctx, 1 if on else 0), "set_profile")

    def event_profile(self):
        ms = ctypes.c_double()
        n = ctypes.c_uint64()
        _lib.check(self.L.bpe_gpu_event_profile(self.ctx, ctypes.byref(ms), ctypes.byref(n)), "event_profile")
        return ms.value, n.value

    def kernel_profile(self):
        name = ctypes.c_char_p()
        ms = ctypes.c_double()
        by = ctypes.c_double()
        n = ctypes.c_uint64()
        _lib.check(self.L.bpe_gpu_kernel_profile(self.ctx, ctypes.byref(name), ctypes.byref(ms), ctypes.byref(by),
                                                 ctypes.byref(n)), "kernel_profile")
        return (name.value or b"").decode(), ms.value, by.value, n.value


class ShardGroup:
    """Corpus-sharded training (bpe_gpu.h group API).

    ShardGroup(device, local_shards=K)           K shards on one device
    ShardGroup(device, nranks=N, rank=r, comm_id=id)  one shard per rank, RCCL
    Shards hold contiguous slices of the corpus in order; merges are the same
    on every shard and the corpus ids are the shards' ids concatenated."""

    P2P_HANDLE_BYTES = 64  # bpe_gpu.h BPE_GPU_P2P_HANDLE_BYTES

    def __init__(self, device=0, local_shards=1, nranks=1, rank=0, comm_id=None, p2p_max_merges=None):
        """p2p_max_merges: one shard per rank over P2P mailboxes (bpe_gpu_group_create_p2p);
        then gather every rank's .p2p_handle in rank order and call p2p_connect()."""
        self.L = _lib.load()
        self.g = ctypes.c_void_p()
        self.p2p_handle = None
        if p2p_max_merges is not None:
            h = ctypes.create_string_buffer(self.P2P_HANDLE_BYTES)
            _lib.check(self.L.bpe_gpu_group_create_p2p(int(device), int(nranks), int(rank), int(p2p_max_merges),
                                                       h, self.P2P_HANDLE_BYTES, ctypes.byref(self.g)),
                       "group_create_p2p")
            self.p2p_handle = h.raw
        else:
            cid = None
            if comm_id is not None:
                cid = ctypes.create_string_buffer(bytes(comm_id), len(comm_id))
            _lib.check(self.L.bpe_gpu_group_create(int(device), int(local_shards), int(nranks), int(rank),
                                                   cid, ctypes.byref(self.g)), "group_create")
        k, n, f = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.check(self.L.bpe_gpu_group_shards(self.g, ctypes.byref(k), ctypes.byref(n), ctypes.byref(f)), "shards")
        self.local_shards, self.nshards, self.first_shard = k.value, n.value, f.value

    def p2p_connect(self, handles):
        """handles: every rank's p2p_handle, in rank order"""
        hs = b"".join(bytes(h) for h in handles)
        buf = ctypes.create_string_buffer(hs, len(hs))
        _lib.check(self.L.bpe_gpu_group_p2p_connect(self.g, buf, self.P2P_HANDLE_BYTES), "p2p_connect")

    def transport(self):
        """'local' (one device), 'rccl' or 'p2p'"""
        v = ctypes.c_int()
        _lib.check(self.L.bpe_gpu_group_transport(self.g, ctypes.byref(v)), "transport")
        return ("local", "rccl", "p2p")[v.value]

    def close(self):
        if self.g:
            self.L.bpe_gpu_group_destroy(self.g)
            self.g = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load(self, k, data: bytes):
        buf = np.frombuffer(data, dtype=np.uint8)
        _lib.check(self.L.bpe_gpu_group_load(self.g, int(k), buf.ctypes.data_as(ctypes.c_void_p), buf.size), "load")

    def load_split(self, data: bytes, cuts):
        """local mode: shard k gets data[cuts[k]:cuts[k+1]]"""
        for k in range(self.local_shards):
            self.load(k, data[cuts[k]:cuts[k + 1]])

    def synth(self, k, seed, n, offset=0):
        _lib.check(self.L.bpe_gpu_group_synth(self.g, int(k), int(seed), int(n), int(offset)), "synth")

    def train(self, max_merges=-1):
        m = ctypes.c_size_t(0)
        _lib.check(self.L.bpe_gpu_group_train(self.g, int(max_merges), ctypes.byref(m)), "group_train")
        return m.value

    def encode(self, merges):
        m = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1)
        _lib.check(self.L.bpe_gpu_group_encode(self.g, m.ctypes.data_as(ctypes.c_void_p), m.size // 2), "group_encode")

    def merges(self):
        cnt = ctypes.c_size_t(0)
        _lib.check(self.L.bpe_gpu_group_fetch_merges(self.g, None, 0, ctypes.byref(cnt)), "fetch_merges")
        out = np.zeros(2 * max(cnt.value, 1), dtype=np.uint32)
        _lib.check(self.L.bpe_gpu_group_fetch_merges(self.g, out.ctypes.data_as(ctypes.c_void_p), cnt.value,
                                                     ctypes.byref(cnt)), "fetch_merges")
        return out[: 2 * cnt.value].reshape(-1, 2)

    def ids(self, k):
        n = ctypes.c_size_t(0)
        _lib.check(self.L.bpe_gpu_group_fetch_ids(self.g, int(k), None, 0, ctypes.byref(n)), "fetch_ids")
        out = np.zeros(max(n.value, 1), dtype=np.uint32)
        _lib.check(self.L.bpe_gpu_group_fetch_ids(self.g, int(k), out.ctypes.data_as(ctypes.c_void_p), n.value,
                                                  ctypes.byref(n)), "fetch_ids")
        return out[: n.value]

    def ids_count(self, k):
        n = ctypes.c_size_t(0)
        _lib.check(self.L.bpe_gpu_group_fetch_ids(self.g, int(k), None, 0, ctypes.byref(n)), "fetch_ids")
        return n.value

    def ids_range(self, k, first, count):
        """ids [first, first + count) of local shard k"""
        out = np.zeros(max(int(count), 1), dtype=np.uint32)
        _lib.check(self.L.bpe_gpu_group_fetch_ids_range(self.g, int(k), int(first), out.ctypes.data_as(ctypes.c_void_p),
                                                        int(count)), "fetch_ids_range")
        return out[: int(count)]

    def all_ids(self):
        return np.concatenate([self.ids(k) for k in range(self.local_shards)])

    def stats(self):
        st = GpuStats()
        _lib.check(self.L.bpe_gpu_group_get_stats(self.g, ctypes.byref(st)), "stats")
        return st.as_dict()

    def ids_checksum(self, base=0):
        """(checksum, n_ids) of the local shards' ids, the first at global index base"""
        s, n = ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self.L.bpe_gpu_group_ids_checksum(self.g, int(base), ctypes.byref(s), ctypes.byref(n)),
                   "ids_checksum")
        return s.value, n.value

    def kernel_profile(self, k=0):
        name = ctypes.c_char_p()
        ms = ctypes.c_double()
        by = ctypes.c_double()
        n = ctypes.c_uint64()
        _lib.check(self.L.bpe_gpu_group_kernel_profile(self.g, int(k), ctypes.byref(name), ctypes.byref(ms),
                                                       ctypes.byref(by), ctypes.byref(n)), "kernel_profile")
        return (name.value or b"").decode(), ms.value, by.value, n.value

    def graph_captured(self):
        v = ctypes.c_int()
        _lib.check(self.L.bpe_gpu_group_exchange_mode(self.g, ctypes.byref(v)), "exchange_mode")
        return bool(v.value)


def comm_id():
    """RCCL unique id (rank 0), to be passed to every rank's ShardGroup"""
    L = _lib.load()
    buf = ctypes.create_string_buffer(128)
    _lib.check(L.bpe_gpu_comm_id(buf, 128), "comm_id")
    return buf.raw


def shard_halo(records, me, a):
    """halo of shard `me` from the (nshards, 16) uint32 edge records (pure host function)"""
    L = _lib.load()
    rec = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, 16)
    out = np.zeros(8, dtype=np.uint32)
    _lib.check(L.bpe_gpu_shard_halo(rec.ctypes.data_as(ctypes.c_void_p), rec.shape[0], int(me), int(a),
                                    out.ctypes.data_as(ctypes.c_void_p)), "shard_halo")
    return {"HL": [int(x) for x in out[0:3]], "HR": [int(x) for x in out[3:6]], "hlrun": int(out[6]),
            "myidx": int(out[7])}


def docs_window(offsets, n, core, halo, w):
    """window w of the document encoder over a batch of n bytes (pure host
    function, bpe_gpu_docs_window): bytes [L, R), whether the neighbour beyond
    each end exists (lunk / runk), the first document with offset >= L and the
    document starts in [L, R]"""
    L = _lib.load()
    off = _doc_offsets(offsets)
    if off.size < 1:
        raise BpeError("docs_window: offsets must hold ndocs + 1 entries")
    out = np.zeros(8, dtype=np.uint64)
    _lib.check(L.bpe_gpu_docs_window(off.ctypes.data_as(ctypes.c_void_p), off.size - 1, int(n), int(core), int(halo),
                                     int(w), out.ctypes.data_as(ctypes.c_void_p)), "docs_window")
    return {"L": int(out[0]), "R": int(out[1]), "lunk": bool(out[2]), "runk": bool(out[3]), "first_doc": int(out[4]),
            "doc_starts": int(out[5])}


def device_count():
    L = _lib.load()
    n = ctypes.c_int(0)
    L.bpe_gpu_device_count(ctypes.byref(n))
    return n.value


def device_pci(device):
    """PCI bus id of a visible device (its identity across processes)"""
    L = _lib.load()
    buf = ctypes.create_string_buffer(64)
    _lib.check(L.bpe_gpu_device_pci(int(device), buf, 64), "device_pci")
    return buf.value.decode()


def peer_access(device, peer):
    """True when `device` can access `peer`'s memory directly"""
    L = _lib.load()
    ok = ctypes.c_int(0)
    _lib.check(L.bpe_gpu_peer_access(int(device), int(peer), ctypes.byref(ok)), "peer_access")
    return bool(ok.value)
