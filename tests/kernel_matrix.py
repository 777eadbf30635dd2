"""The one case table of the conv3x3 and linear kernel families (csrc/p2p_conv.hip, csrc/p2p_linear.hip):
every compiled instantiation at the smallest shape that reaches it.  Plain data, no torch and no GPU;
not collected.  tests/test_select_instances.py proves on the CPU, from what csrc/p2p_select.h answers,
that the rows reach every instantiation; tests/test_gpu_conv_matrix.py and tests/test_gpu_linear_matrix.py
run every row in bf16 and f16 against the f64 formula.  A new tile shape, loop, form or epilogue
extends the lists below, and test_select_instances.py's product with them.

The constants are include/p2p_hip.h's and p2p_select.h's values (the GPU tests assert that p2p_amd._hip
has the same ones)."""
import itertools

SAME, UP2, DOWN2 = 0, 1, 2                               # P2P_CONV_*
LOOP_AUTO, LOOP_TILE, LOOP_PIPE128, LOOP_PIPE256 = 0, 1, 2, 3   # p2p::ConvLoop
LIN_BIAS, LIN_GEGLU, LIN_RESIDUAL = 0, 1, 2              # P2P_LINEAR_*

FORM_NAMES = {SAME: "same", UP2: "up2", DOWN2: "down2"}
LOOP_NAMES = {LOOP_TILE: "tile", LOOP_PIPE128: "pipe128", LOOP_PIPE256: "pipe256"}
LIN_NAMES = {LIN_BIAS: "bias", LIN_GEGLU: "geglu", LIN_RESIDUAL: "residual"}

# ---------------------------------------------------------------------------- 3x3 convolution
# Every row has an 8 x 8 OUTPUT map and n = 3: M = 192 is one 128-pixel tile plus a 64-pixel tail (the
# 256-pixel ring: one tile with a 64-pixel hole), and two images share a tile.
CONV_N = 3
CONV_INPUT_MAP = {SAME: (8, 8), UP2: (4, 4), DOWN2: (16, 16)}

# (c_in, c_out) without and with a K split, and the loops forced on it, per tile (bk, bn).  At an 8 x 8
# output: 64 -> 160 split 1, 128 -> 160 split 2; 64 -> 96 split 1 with a c_out tail, 128 -> 96 split 2;
# 32 -> 32 split 1, 96 -> 32 split 3 (ranges of 9 steps each).
CONV_TILES = [
    # (c_in one launch, c_in split, c_out, loops)
    (64, 128, 96, (LOOP_TILE,)),                                  # bk 64, bn 128
    (32, 96, 32, (LOOP_TILE,)),                                   # bk 32, bn 128
    (64, 128, 160, (LOOP_TILE, LOOP_PIPE128, LOOP_PIPE256)),      # bk 64, bn 160
]

# rows: (form, n, input h, input w, c_in, c_out, bias, forced loop)
CONV_ROWS = [
    (form, CONV_N, *CONV_INPUT_MAP[form], c_split if split else c_one, c_out, bias, loop)
    for form in (SAME, UP2, DOWN2)
    for c_one, c_split, c_out, loops in CONV_TILES
    for loop in loops
    for split in (False, True)
    for bias in (False, True)
]


def conv_id(row):
    form, n, h, w, c_in, c_out, bias, loop = row
    return f"{FORM_NAMES[form]}-{c_in}to{c_out}-{'bias' if bias else 'nobias'}-{LOOP_NAMES[loop]}"


# ---------------------------------------------------------------------------- linear
# (K, N) of the BIAS and RESIDUAL forms at M = 136 (a 128-row tile and an 8-row tail):
#   64, 96      bk 64, bn 128, split 1          1088, 96    bk 64, bn 128, split 2 (17 steps: 8 and 9)
#   96, 96      bk 32, bn 128, split 1          544, 96     bk 32, bn 128, split 2 (17 steps)
#   64, 160     bk 64, bn 160, split 1          1088, 160   bk 64, bn 160, split 2
LIN_KN = [(64, 96), (1088, 96), (96, 96), (544, 96), (64, 160), (1088, 160)]
# one row, below half a tile, odd: on the two bn 160 shapes and on 1088 -> 328 (three column tiles of
# 128, the last 72 wide; split 2)
LIN_SMALL_M = [1, 8, 77]
LIN_SMALL_KN = [(64, 160), (1088, 160), (1088, 328)]
# GEGLU (M, K, D): D = 72 is a 64-column tile and one of 8 columns, in which wave column 1 (tile
# columns 32 .. 63) holds no valid output column; K = 96 is bk 32; D = 8 at M = 8 is all tail
LIN_GEGLU_MKD = [(136, 64, 72), (136, 96, 72), (8, 64, 8)]

# rows: (form, M, K, N, bias, strided, p_out) -- N is D for the GEGLU form; strided: x and res are
# column slices of wider tensors, as test_gpu_linear.operands makes them; p_out: GEGLU only
LINEAR_ROWS = [
    (form, m, k, n, bias, strided, False)
    for form in (LIN_BIAS, LIN_RESIDUAL)
    for m, k, n in [(136, k, n) for k, n in LIN_KN] + [(m, k, n) for k, n in LIN_SMALL_KN for m in LIN_SMALL_M]
    for bias, strided in itertools.product((False, True), repeat=2)
] + [
    (LIN_GEGLU, m, k, d, bias, False, p_out)
    for m, k, d in LIN_GEGLU_MKD
    for bias, p_out in itertools.product((False, True), repeat=2)
]


def linear_id(row):
    form, m, k, n, bias, strided, p_out = row
    return (f"{LIN_NAMES[form]}-{m}x{k}x{n}-{'bias' if bias else 'nobias'}-{'strided' if strided else 'dense'}"
            + ("-p_out" if p_out else ""))
