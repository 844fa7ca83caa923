/*
 * bpe_split_presets.h -- the preset split rules of bpe_gpu.h (BPE_SPLIT_*) in one list: which numbers are
 * presets and which of them two tables express.  Read by the library's C files and by the engine's host code
 * (csrc/pieces.hip); not part of the API.  A new preset is one line here (and its name in api.py).
 */
#ifndef BPE_SPLIT_PRESETS_H
#define BPE_SPLIT_PRESETS_H

#include <stddef.h>

#include "../../include/bpe_gpu.h"

struct split_preset {
    int id;
    const char *name; /* as bpe_gpu.h spells it, for messages */
    int has_tables;   /* bpe_gpu_split_rule fills cls / brk; 0: a marking kernel of its own */
};

/* the line of `preset`, or NULL: no such preset */
static inline const struct split_preset *split_preset_find(int preset)
{
    static const struct split_preset all[] = {
        {BPE_SPLIT_LINES, "BPE_SPLIT_LINES", 1},
        {BPE_SPLIT_WORDS, "BPE_SPLIT_WORDS", 1},
        {BPE_SPLIT_GPT2, "BPE_SPLIT_GPT2", 0},
        {BPE_SPLIT_GPT2_UNICODE, "BPE_SPLIT_GPT2_UNICODE", 0},
        {BPE_SPLIT_CL100K, "BPE_SPLIT_CL100K", 0},
    };
    for (size_t k = 0; k < sizeof all / sizeof all[0]; k++)
        if (all[k].id == preset) return &all[k];
    return NULL;
}

#endif
