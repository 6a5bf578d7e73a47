"""The launch forms of the patch embeddings: one plain table of cases per form, and a Python restatement of the host rules
that decide which kernel body, how many k-splits, which row plan and which argument order a launch gets.

tests/test_host_embed_forms.py classifies every case with these rules and checks that the table as a whole reaches each
form; tests/test_gpu_embed_forms.py runs every case against the float64 references of tests/embed_ref.py and compares the
restated rules with the library's own answers where it exports them (m2m_embed_fwd_splits, m2m_embeds_wgrad_form).

Restated from csrc/embed_fwd.h (embed_fwd_fast_ok, the stage range of a k-split), csrc/embed.hip (m2m_embed_fwd_splits, the
`first` of launch_embed_fwd_group) and csrc/embed_wgrad.h (embed_wgrad_plan, embed_wgrad_group_args_fast, the `first` of
embed_wgrad_group_args).
"""
from collections import namedtuple

EMB_KS, EMB_FKS = 128, 256      # k extent of a stage: generic body, fast body
EBM, EFK = 32, 32               # row-group form: token rows per tile; single-owner form: pixel columns per workgroup
BM, WPAIR = 16, 32              # rows of a chain tile; rows of an operand-image pair

Geom = namedtuple("Geom", "Cin H W ph pw")


def geomK(g):
    return g.Cin * g.ph * g.pw


def geomN(g):
    return (g.H // g.ph) * (g.W // g.pw)


def kblock(prec):
    return 32 if prec == "bf16" else 16


def padK(K, prec):
    kb = kblock(prec)
    return (K + kb - 1) // kb * kb


# ---- forward ----------------------------------------------------------------------------------------------------------
def fwd_fast_ok(g, prec, align=16):
    """embed_fwd_fast_ok; `align`: the largest power of two (up to 16) that divides the input's address."""
    return prec == "bf16" and g.pw % 8 == 0 and g.W % 4 == 0 and geomK(g) >= 8 and align % 16 == 0


def fwd_splits(g, prec):
    """m2m_embed_fwd_splits (without the diagnostic override)."""
    return 2 if fwd_fast_ok(g, prec) and padK(geomK(g), prec) >= 4 * EMB_FKS else 1


def split_stages(g, nsplit):
    """[(first stage, end stage)] of every part of a k-split fast forward; begin >= end is an empty part."""
    nst_all = (padK(geomK(g), "bf16") + EMB_FKS - 1) // EMB_FKS
    per = (nst_all + nsplit - 1) // nsplit
    return [(s * per, min(nst_all, s * per + per)) for s in range(nsplit)]


def fwd_first(g0, g1, prec):
    """launch_embed_fwd_group: index of the embedding dispatched first (the one with the larger padded K)."""
    return 1 if padK(geomK(g1), prec) > padK(geomK(g0), prec) else 0


# ---- weight gradient, row-group form --------------------------------------------------------------------------------------
Plan = namedtuple("Plan", "M N nchunks groups tpg ntiles last")


def wgrad_plan(g, B, target):
    """embed_wgrad_plan(target): 64-column chunks x row groups of `tpg` 32-row tiles; `last`: tiles of the last group."""
    N = geomN(g)
    M = B * N
    nchunks = (geomK(g) + 63) // 64
    ntiles = (M + EBM - 1) // EBM
    groups = (target + nchunks - 1) // nchunks
    groups = min(groups, ntiles // 4)
    groups = max(groups, 1)
    tpg = (ntiles + groups - 1) // groups
    groups = (ntiles + tpg - 1) // tpg
    return Plan(M, N, nchunks, groups, tpg, ntiles, ntiles - (groups - 1) * tpg)


def wgrad_first(g0, g1, B, target):
    """embed_wgrad_group_args: index of the embedding dispatched first (more row tiles per workgroup)."""
    return 1 if wgrad_plan(g1, B, target).tpg > wgrad_plan(g0, B, target).tpg else 0


def wgrad_target(D, merged):
    """Workgroups the plan aims at: 256 in the embeddings' own launches, 512 (128 at hidden_dim 256) inside m2m_towers_wgrad."""
    return (128 if D >= 256 else 512) if merged else 256


# ---- weight gradient, single-owner form -----------------------------------------------------------------------------------
Owner = namedtuple("Owner", "npairs rpt nchunks vec2")


def wgrad_owner_args(g, B, align=16):
    """embed_wgrad_group_args_fast for an embedding whose tower is on the fused path (N <= 8, 16 % ... whole samples per tile)."""
    N, K = geomN(g), geomK(g)
    spw = BM // N
    nchain = (B + spw - 1) // spw
    vec2 = g.pw % 2 == 0 and g.W % 2 == 0 and (g.H * g.W) % 2 == 0 and K % 2 == 0 and align % 8 == 0
    return Owner((nchain * BM + WPAIR - 1) // WPAIR, spw * N, (K + EFK - 1) // EFK, vec2)


def wgrad_owner_ok(g, prec, D, B):
    N = geomN(g)
    return prec == "bf16" and N <= 8 and D <= 128 and B * g.Cin * g.H * g.W < (1 << 31)


def owner_waves(D):
    """Waves of the merged weight-gradient launch's workgroups (bf16): 5 at hidden_dim 128, else 4."""
    return 5 if D == 128 else 4


# ---- geometries ----------------------------------------------------------------------------------------------------------
G = {
    "c2_6x10_p3x5": Geom(2, 6, 10, 3, 5),           # K 30   N 4   ph < pw
    "c3_12x12_p4": Geom(3, 12, 12, 4, 4),           # K 48   N 9
    "c1_10x35_p10x7": Geom(1, 10, 35, 10, 7),       # K 70   N 5   ph > pw, odd W
    "c1_34x17_p17": Geom(1, 34, 17, 17, 17),        # K 289  N 2
    "c1_13x20_p13x10": Geom(1, 13, 20, 13, 10),     # K 130  N 2   just over a 128-wide stage
    "c1_15x8_p5x8": Geom(1, 15, 8, 5, 8),           # K 40   N 3   fast: one partly valid stage
    "c1_32x16_p16": Geom(1, 32, 16, 16, 16),        # K 256  N 2   fast: exactly one stage
    "c1_33x16_p33x8": Geom(1, 33, 16, 33, 8),       # K 264  N 2   fast: one stage + 8
    "c1_32x40_p16x40": Geom(1, 32, 40, 16, 40),     # K 640  N 2   fast: 3 stages
    "c4_16x32_p16": Geom(4, 16, 32, 16, 16),        # K 1024 N 2   fast: 4 stages
    "c1_16x24_p16x8": Geom(1, 16, 24, 16, 8),       # K 128  N 3
    "c1_7x28_p7x4": Geom(1, 7, 28, 7, 4),           # K 28   N 7
    "c3_12x12_p6": Geom(3, 12, 12, 6, 6),           # K 108  N 4
    "c2_16x24_p8": Geom(2, 16, 24, 8, 8),           # K 128  N 6
    "c1_16x8_p16x8": Geom(1, 16, 8, 16, 8),         # K 128  N 1
    "c1_16x16_p4x8": Geom(1, 16, 16, 4, 8),         # K 32   N 8
    "c1_16x8_p8": Geom(1, 16, 8, 8, 8),             # K 64   N 2
    "c1_16x16_p8": Geom(1, 16, 16, 8, 8),           # K 64   N 4
}

# ---- the forms ------------------------------------------------------------------------------------------------------------
# (prec, D, geometry, B): m2m_embed_forward on an aligned input
FWD_SINGLE = [
    ("fp32", 32, "c2_6x10_p3x5", 7),               # K < 128, K % 16 != 0, M = 28
    ("bf16", 64, "c3_12x12_p4", 31),               # Cin 3, K % 32 != 0, M = 279
    ("fp32", 128, "c1_10x35_p10x7", 5),            # M = 25
    ("bf16", 128, "c1_10x35_p10x7", 5),
    ("fp32", 256, "c1_34x17_p17", 3),              # K = 288 + 1, M = 6 < 16
    ("bf16", 256, "c1_34x17_p17", 3),
    ("fp32", 64, "c1_13x20_p13x10", 9),            # K = 130: Kp 144
    ("bf16", 32, "c1_13x20_p13x10", 9),            # Kp 160
    # fast body
    ("bf16", 32, "c1_15x8_p5x8", 37),              # waves 2..7 own no d-tile and no valid k
    ("bf16", 256, "c1_32x16_p16", 5),              # two d-tiles per wave
    ("bf16", 64, "c1_33x16_p33x8", 9),
    ("bf16", 128, "c1_32x40_p16x40", 40),
    ("bf16", 128, "c4_16x32_p16", 7),
]

# (prec, D, (geometry 0, geometry 1), B, [nsplits to run: both embeddings get the same]): m2m_embeds_forward, in BOTH argument orders
FWD_GROUP = [
    ("bf16", 128, ("c1_32x40_p16x40", "c4_16x32_p16"), 40, [1, 2, 3, 4]),
    ("bf16", 32, ("c1_15x8_p5x8", "c1_32x16_p16"), 11, [1, 2, 4]),
    ("bf16", 256, ("c1_33x16_p33x8", "c1_34x17_p17"), 3, [1, 3]),        # fast + generic body in one launch
    ("fp32", 64, ("c3_12x12_p4", "c1_13x20_p13x10"), 6, [1]),
]

# (prec, D, (geometry 0, geometry 1), B, (nsplits 0, nsplits 1)): generic body asked for parts (inputs offset by 4 bytes)
FWD_GENERIC_PARTS = [
    ("bf16", 64, ("c1_15x8_p5x8", "c1_32x16_p16"), 11, (3, 2)),
    ("fp32", 32, ("c2_6x10_p3x5", "c1_16x8_p8"), 7, (2, 4)),
]

# (D, geometry, B, parts): the consumer of the parts (m2m_towers_forward, fused pair, eval mode); both towers take the geometry
CONSUMER = [(128, "c4_16x32_p16", 7, 2), (64, "c1_32x40_p16x40", 9, 3), (32, "c4_16x32_p16", 5, 4)]

# (prec, D, channel_dim, (geometry 0, geometry 1 or None), B): embeddings inside the tower forward launch; None: that tower
# takes a given x0 (embeds[i] == NULL) and its partner's N.  The two towers are one block deep, token_dim 8.
TOWER_FWD = [
    ("fp32", 32, 32, ("c2_6x10_p3x5", "c3_12x12_p6"), 7),        # small-LDS launch: 32592 bytes before the fix (N = 4)
    ("fp32", 32, 20, ("c1_16x16_p4x8", None), 3),                 # small-LDS launch: 33104 bytes before the fix (N = 8)
    ("bf16", 64, 32, ("c1_16x8_p16x8", "c1_16x8_p8"), 19),       # N 1 + N 2, fast body
    ("bf16", 128, 64, ("c1_34x17_p17", "c4_16x32_p16"), 5),      # N 2 generic + N 2 fast
    ("bf16", 32, 32, ("c1_16x16_p4x8", "c1_16x16_p4x8"), 3),     # N 8, fast body
    ("fp32", 64, 40, (None, "c1_16x16_p8"), 17),                 # N 4, the first tower given its x0
]

# (prec, D, geometry, B): row-group weight gradient through m2m_embed_wgrad and the merged launch with nembeds = 1
WGRAD_ROWS = [
    ("fp32", 32, "c3_12x12_p4", 31),               # 9 tiles, tpg 5, last group 4; K 48 < 64
    ("bf16", 64, "c1_16x24_p16x8", 113),           # 11 tiles, 2 chunks, last group 5
    ("fp32", 64, "c2_6x10_p3x5", 7),               # one tile, groups 1
    ("bf16", 32, "c1_10x35_p10x7", 31),            # K 70: two chunks, the second 6 wide; groups 1
    ("bf16", 128, "c1_34x17_p17", 3),              # 5 chunks
    ("fp32", 256, "c3_12x12_p4", 31),
]
# (prec, D, (geometry 0, geometry 1), B): m2m_embeds_wgrad and the merged launch with nembeds = 2, in BOTH argument orders
WGRAD_ROWS_GROUP = [
    ("fp32", 32, ("c3_12x12_p4", "c2_6x10_p3x5"), 31),          # tpg 5 against 4
    ("bf16", 64, ("c1_16x24_p16x8", "c1_10x35_p10x7"), 113),    # tpg 6 against 5
]

# (D, (geometry 0, geometry 1), B, overwrite, (input 0 offset by 4 bytes, input 1 offset)): single-owner weight gradient, bf16
WGRAD_OWNER = [
    (32, ("c1_15x8_p5x8", "c3_12x12_p6"), 37, True, (False, False)),        # N 3 (rpt 15), N 4; K 40, K 108
    (64, ("c3_12x12_p6", "c1_15x8_p5x8"), 5, False, (False, False)),        # npairs 1
    (128, ("c1_10x35_p10x7", "c1_7x28_p7x4"), 20, True, (False, False)),    # N 5 (odd pw: vec2 off), N 7 (rpt 14, K 28)
    (32, ("c1_7x28_p7x4", "c1_10x35_p10x7"), 9, False, (False, False)),     # npairs 3 and 2
    (64, ("c2_16x24_p8", "c1_16x16_p4x8"), 21, True, (False, False)),       # N 6, N 8: npairs 6 and 11
    (128, ("c1_16x8_p16x8", "c1_16x8_p16x8"), 100, True, (False, True)),    # N 1; the second input 4 bytes off: vec2 off
    (32, ("c1_16x8_p16x8", "c1_16x8_p8"), 170, False, (False, False)),      # N 1: npairs 6; N 2: npairs 11
]
