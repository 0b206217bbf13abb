"""Shape tables of tests/test_norm_forms_gpu.py (plain data, no GPU, no fixtures).

tests/test_kernel_forms_cpu.py asks the built libraries which kernel form each row takes (df_test_groupnorm_form /
df_test_attention_form: the functions the launchers dispatch on) and asserts that every form is reached, so a row that is the
only cover of a form cannot be deleted, and a form added to a launcher without a row here fails on the CPU.
"""

# ---- GroupNorm: (mode, N, HW, C, silu, eps, nslab, c_own)
#   mode "plain": x is the tensor;  "slabs": x is the first of nslab split-K slabs of the producing conv (+ bias + per-sample bias);
#   "own": channels [0, c_own) are the norm's own producer's slabs (+ bias + residual), written back to x.
# Every case runs with ld > C, ldo > C, raw_out and sentinel-filled outputs.  N = 8 takes the register kernel's sample-major block
# order (all groups of a sample on one XCD), any other N the group-major one.
_GN_REG = [
    # (N, HW, C)                       PER  what
    (2, 16, 1280),                   # 1    lowest UNet level
    (8, 16, 1280),                   # 1    CFG batch of 8
    (3, 1, 320),                     # 1    one-row tensor
    (2, 256, 320),                   # 2    model shape 320 x 256
    (1, 257, 320),                   # 2    HW odd: second pass one row short
    (2, 64, 1280),                   # 2
    (2, 256, 640),                   # 3
    (1, 254, 640),                   # 3    ragged last pass
    (2, 256, 960),                   # 4    model shape 960 x 256
    (8, 250, 960),                   # 4    ragged, sample-major blocks, group 21 across the 640 | 320 concat boundary
    (2, 1024, 320),                  # 6
    (1, 1021, 320),                  # 6    ragged
    (1, 1500, 320),                  # 8    ragged (8 x 188 = 1504)
    (1, 2048, 128),                  # 8
    (2, 1024, 640),                  # 12   model shape 640 x 1024
    (1, 1000, 640),                  # 12   ragged
    (2, 1024, 960),                  # 16   model shape 960 x 1024: up-path concat norm
    (1, 1023, 960),                  # 16   ragged
    (1, 1090, 960),                  # 20   ragged
    (1, 5461, 192),                  # 20
]
_GN_PLAIN_ONLY = [
    (1, 1024, 1280),                 # streaming: 20480 items, C not 128 / 256 / 512
    (2, 17001, 64),                  # streaming: one channel pair per group, odd HW
    (1, 9000, 192),                  # streaming
    (1, 8192 + 77, 128),             # chunked, ragged last chunk
    (1, 16384 + 100, 256),           # chunked
    (2, 4096 + 33, 512),             # chunked
    (1, 40000, 128),                 # chunked, many chunks
]


GN_MAX_ELEMS = 65536 * 128      # the largest GroupNorm tensor of tests/test_kernels_gpu.py; slabs included, no case holds more


def _gn_cases():
    out = []
    cap = lambda want, N, HW, C: max(2, min(want, GN_MAX_ELEMS // (N * HW * C)))
    for i, (N, HW, C) in enumerate(_GN_REG + _GN_PLAIN_ONLY):
        out.append(("plain", N, HW, C, i % 2, 1e-5 if i % 3 else 1e-6, 0, 0))
    for i, (N, HW, C) in enumerate(_GN_REG):
        out.append(("slabs", N, HW, C, (i + 1) % 2, 1e-5, cap((2, 3, 5, 8, 17)[i % 5], N, HW, C), 0))
    for i, (N, HW, C) in enumerate(_GN_REG):
        # the producer owns all channels, or the first two thirds / half of a concat buffer (960 = 640 + 320, 1280 = 640 + 640 ...)
        c_own = C if i % 2 == 0 else {320: 160, 640: 320, 960: 640, 1280: 640, 128: 64, 192: 128}[C]
        out.append(("own", N, HW, C, 1, 1e-5, cap((2, 4, 3, 16, 7)[i % 5], N, HW, C), c_own))
    return out


GN_CASES = _gn_cases()
GN_FORMS_REG = (1, 2, 3, 4, 6, 8, 12, 16, 20)
GN_STREAMING, GN_CHUNKED, GN_REFUSED = -1, -2, -3

# ---- LayerNorm: (rows, C, ld) -- one instantiation per C = 64 NV, NV = 1 .. 32; rows that are and are not multiples of the four
# rows a block takes, including one row; ld == C on every fifth width, ld > C elsewhere.
_LN_ROWS = (1, 2, 3, 4, 5, 7, 8, 13, 64, 77)
LN_CASES = [(_LN_ROWS[nv % len(_LN_ROWS)], 64 * nv, 64 * nv + (0 if nv % 5 == 0 else 12 if nv % 2 else 64)) for nv in range(1, 33)]
LN_CASES += [(1024, 320, 960), (513, 1280, 1288), (1, 2048, 2100)]

# ---- attention: (N, heads, D, Tq, Tk, fused)
#   fused: Q and K are the column ranges [0, C) and [C, 2C) of ONE [N*T][2C] buffer (the fused-QKV output), ldq = ldk = 2C; Tq == Tk.
# Every case has ldo > heads * D with a sentinel in the pad columns and in a guard row, and NaN-poisoned V^T padding.
ATTN_DIMS = (16, 24, 32, 40, 48, 56, 64, 72, 80, 96, 112, 128, 160, 192)
ATTN_FORMS = {66: "<D,4,2>", 65: "<D,4>", 33: "<D,2>", 17: "<D,1>"}


def _attn_cases():
    out = []
    for D in ATTN_DIMS:
        out += [(2, 2, D, 192, 192, 1),      # <D,4,2> for D <= 80 (else <D,4>): ragged second query block (192 = 128 + 64)
                (1, 2, D, 200, 200, 1),      # <D,4>: Tk = 200 is no multiple of 64 or 32; ragged query block and ragged wave
                (2, 2, D, 77, 77, 1),        # <D,2>: ragged second block, Tk no multiple of 32
                (2, 3, D, 19, 19, 1),        # <D,1>
                (1, 2, D, 129, 33, 0),       # <D,4>: one query row in the second block, 33 context tokens
                (1, 3, D, 65, 45, 0)]        # <D,2>: one query row in the second wave
        if D <= 80:
            out.append((1, 2, D, 129, 64, 0))      # <D,4,2> with separate Q / K buffers
    return out


ATTN_CASES = _attn_cases()
