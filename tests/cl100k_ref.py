"""BPE_SPLIT_CL100K restated in Python, character by character as bpe_gpu.h states it: the text decoded
with errors="surrogateescape" (every byte in no well-formed sequence is a character of its own, class
P), the classes of api.unicode_class with \\r and \\n split off as R, and one decision per character
from its neighbours, its index in a run of numbers and the white-space run around it.  It shares no
code with src/bpe_split_preset.c; tests/test_split_cl100k_host.py holds both to the regular expression
where the regex module is installed.  Random access and rescans: for short texts only."""
from functools import lru_cache

from llmtokenizer_amd import api

PATTERN = (r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*"
           r"|\s*[\r\n]+|\s+(?!\S)|\s+")


@lru_cache(maxsize=None)
def char_class(ch):
    """R S W L N or P"""
    if ch in "\r\n":
        return "R"
    if 0xDC80 <= ord(ch) <= 0xDCFF:  # an escaped byte
        return "P"
    return api.unicode_class(ord(ch))


def fold(ch):
    """the letter a contraction reads: A-Z fold, U+017F is an s; "" for everything else"""
    if ch == "ſ":
        return "s"
    return ch.lower() if ("a" <= ch <= "z" or "A" <= ch <= "Z") else ""


def char_starts(text):
    """the indices of the characters of text that start a piece"""
    n = len(text)
    K = [char_class(ch) for ch in text]

    def k(i):
        return K[i] if i >= 0 else "R"  # before the text everything reads as R

    def clen(j):
        if j < 0 or text[j] != "'" or k(j - 1) in "PS":
            return 0
        if j + 1 < n and fold(text[j + 1]) in ("s", "t", "m", "d"):
            return 2
        if j + 2 < n and fold(text[j + 1]) + fold(text[j + 2]) in ("re", "ve", "ll"):
            return 3
        return 0

    out = []
    for i in range(n):
        c, p = K[i], k(i - 1)
        if i == 0:
            s = True
        elif c == "N":
            run = 0  # the index of i within its run of numbers
            while i - run - 1 >= 0 and K[i - run - 1] == "N":
                run += 1
            s = run % 3 == 0
        elif c in "RSW":
            if p not in "RSW":
                s = not (p == "P" and c == "R")
            elif c == "R":
                s = False
            else:
                a = i  # the run is [a, q)
                while a > 0 and K[a - 1] in "RSW":
                    a -= 1
                q = i
                while q < n and K[q] in "RSW":
                    q += 1
                s = ((i == q - 1 and q < n)
                     or (p == "R" and "R" not in K[i:q])
                     or (p == "R" and all(x == "R" for x in K[a:i]) and a > 0 and K[a - 1] == "P"))
        elif c == "L":
            if clen(i - 1) >= 2 or clen(i - 2) == 3:
                s = False
            elif clen(i - 2) == 2 or clen(i - 3) == 3:
                s = True
            elif p == "L":
                s = False
            elif p in "NR":
                s = True
            elif p in "SW":
                s = False
            else:
                s = k(i - 2) in "PS"
        else:
            s = p in "LN" or p in "RW"
        if s:
            out.append(i)
    return out


def offsets(data):
    """the byte offsets of the pieces of data, followed by len(data)"""
    text = data.decode("utf-8", "surrogateescape")
    at = [0]
    for ch in text:
        at.append(at[-1] + len(ch.encode("utf-8", "surrogateescape")))
    return [at[i] for i in char_starts(text)] + [len(data)]
