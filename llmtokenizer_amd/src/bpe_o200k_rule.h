/*
 * bpe_o200k_rule.h -- BPE_SPLIT_O200K (bpe_gpu.h) as one automaton, in plain C: what a character does to the
 * state of the piece it is read in, and whether it starts a piece.  The host rule (bpe_split_preset.c) walks it
 * over the text; the engine (csrc/split.hip) folds it into the table its kernels look up, so both sides are
 * this one statement.  Not part of the API.
 *
 * A character is a kind and up to three flags that its neighbours decide (bpe_gpu.h says which); together they
 * are its symbol, O2_SYMBOLS of them.  The state is what the next character has to know of the text before it.
 */
#ifndef BPE_O200K_RULE_H
#define BPE_O200K_RULE_H

#include <stdint.h>

/* kinds: P other text, U l B M the case classes, N numbers, W white space but \r \n, R \r \n, SL '/', AP the
 * apostrophe, X a byte of a special's match (or a text break), CONT a byte inside a well-formed sequence */
enum { O2_P = 0, O2_U, O2_LOW, O2_B, O2_M, O2_N, O2_W, O2_R, O2_SL, O2_AP, O2_X, O2_CONT, O2_KINDS };
/* flags, by kind.  Letters (U l B M): F0 the character ends the letters of a contraction, F1 the character
 * before is W, F2 (U) the character before is B or M and only U follow up to a character that is no letter.
 * W: F0 a start whatever the state, F1 the character before is R.  R: F0 the character before is no white space.
 * P SL AP: F0 the next character is a letter or M, F1 the character before is the space, F2 (AP) the letters of a
 * contraction follow. */
enum { O2_F0 = 16, O2_F1 = 32, O2_F2 = 64, O2_SYMBOLS = 128 };
/* states: FRESH nothing is carried; UB / LB the letters of a word, before / after its first l (or first B after
 * an l); C inside the letters of a contraction; N1 N2 numbers of a piece so far; PU the body of a punctuation
 * piece; PT its tail of \r \n / */
enum { O2_FRESH = 0, O2_UB, O2_LB, O2_C, O2_N1, O2_N2, O2_PU, O2_PT, O2_STATES };

#ifndef O2_FN
#define O2_FN static inline
#endif

/* the state after a character of symbol `sym` read in state `st`; *start: the character starts a piece */
O2_FN int o2_step(int st, int sym, int *start)
{
    const int k = sym & 15, f0 = !!(sym & O2_F0), f1 = !!(sym & O2_F1), f2 = !!(sym & O2_F2);
    const int tail = st == O2_PU || st == O2_PT;
    int s = 0, to = O2_FRESH;
    switch (k) {
    case O2_U: case O2_LOW: case O2_B: case O2_M:
        if (st == O2_C) {
            to = f0 ? O2_FRESH : O2_C;
            break;
        }
        if (k == O2_M && st == O2_PU) {
            to = O2_PU;
            break;
        }
        s = st == O2_UB ? k == O2_U && f2 : st == O2_LB ? k == O2_U : st == O2_FRESH ? !f1 : 1;
        to = k == O2_U ? O2_UB : k == O2_LOW ? O2_LB : st == O2_LB && !s ? O2_LB : O2_UB;
        break;
    case O2_N:
        s = st != O2_N1 && st != O2_N2;
        to = st == O2_N1 ? O2_N2 : st == O2_N2 ? O2_FRESH : O2_N1;
        break;
    case O2_W:
        s = f0 || (f1 && st == O2_PT);
        break;
    case O2_R:
        s = f0 && !tail;
        to = tail ? O2_PT : O2_FRESH;
        break;
    case O2_P: case O2_SL: case O2_AP:
        if (k == O2_AP && f2 && (st == O2_UB || st == O2_LB)) {
            to = O2_C;
            break;
        }
        if (st == O2_PU || (st == O2_PT && k == O2_SL)) {
            to = st;
            break;
        }
        s = !(st == O2_FRESH && f1);
        to = s && f0 ? O2_UB : O2_PU;
        break;
    case O2_CONT:
        to = st;
        break;
    default: /* O2_X: a segment ends before it and begins after it */
        break;
    }
    *start = s;
    return to;
}

/* the two chains read from the right, as one state: bit 0 AU (only U lie between here and a character that is no
 * letter), bit 1 FOL (an R lies ahead in this white-space run).  The state to the left of a character of kind k
 * when `right` is the state to its right.  At the end of the text: O2_BACK_END */
enum { O2_BACK_END = 1 };
O2_FN int o2_back(int right, int k)
{
    if (k == O2_CONT) return right;
    const int au = k == O2_U ? right & 1 : !(k == O2_LOW || k == O2_B || k == O2_M);
    const int fol = k == O2_R ? 2 : k == O2_W ? right & 2 : 0;
    return au | fol;
}

#endif
