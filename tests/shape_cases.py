"""The shape envelope of the module path: one plain table of cases, chosen by the kernel path and the tail each reaches.

tests/test_gpu_shape_envelope.py runs every case forward and backward in fp32 and bf16 against the float64 oracle;
tests/test_host_cpu.py (test_shape_envelope_covers_every_build) classifies every case with the host's dispatch rules and
checks that each kernel build the library instantiates is reached by at least one case.

Fields (unused ones are None):
  name     test id
  kind     "block" (MixerBlock), "fusion" (FusionMixer), "mixer" (MLPMixer: patch embedding), "nopatch"
           (MLPMixerNoPatching: Linear embedding of given tokens), "mlp" (MLP)
  D N T C  hidden_dim, num_patch, token_dim, channel_dim of the tower
  nb       MixerBlocks in the tower
  B        batch
  p        dropout (0.5 selects the kernels' DM_HALF build, any other p > 0 DM_GEN)
  emb      "mixer": (in_channels, (H, W), patch); "nopatch": embedding_dim
  mlp      (input_dim, hidden_dim, num_blocks, output_dim or None)
"""
from collections import namedtuple

Case = namedtuple("Case", "name kind D N T C nb B p emb mlp")


def _c(name, kind, D=None, N=None, T=None, C=None, nb=1, B=2, p=0.0, emb=None, mlp=None):
    return Case(name, kind, D, N, T, C, nb, B, p, emb, mlp)


# largest (nblocks, channel_dim) of the fused path at hidden_dim 128, N = 8, token_dim 32: the fp32 backward launch's LDS
# (tower_bwd.hip BwdLds, 160 KiB) holds 3 blocks up to Cp = 3488; Cp = 3520 is refused (test_unsupported_shapes_are_refused)
LDS_EDGE = dict(D=128, N=8, T=32, nb=3, C=3488)

CASES = [
    # ---- fused path (N <= 8, D <= 128): whole samples per 16-row tile, SPW = 16 // N; NMAX 4 for N <= 4, 8 for N 5..8 ----
    _c("fused_n1_d32_c1_b1", "block", 32, 1, 8, 1, B=1),
    _c("fused_n1_d128_b17", "block", 128, 1, 16, 64, B=17),                   # SPW 16: B = 17 leaves one sample in tile 2
    _c("fused_n2_d64_t24_c31_half", "block", 64, 2, 24, 31, B=9, p=0.5),
    _c("fused_n2_d128_c100_half", "block", 128, 2, 8, 100, B=3, p=0.5),
    _c("fused_n3_d128_t32_c33_gen", "block", 128, 3, 32, 33, B=7, p=0.1),   # SPW 5: 15 of 16 rows used
    _c("fused_n4_d32_gen", "block", 32, 4, 16, 64, B=5, p=0.1),
    _c("fused_n3_d64_t24_c100_gen", "block", 64, 3, 24, 100, B=4, p=0.1),
    _c("fused_n4_d64_t32_c33_x2", "fusion", 64, 4, 32, 33, nb=2, B=5),
    _c("fused_n3_d32_c31_x2_half", "fusion", 32, 3, 8, 31, nb=2, B=6, p=0.5),
    _c("fused_n5_d32_c100_half", "block", 32, 5, 16, 100, B=5, p=0.5),     # SPW 3
    _c("fused_n5_d128_c50_gen", "block", 128, 5, 8, 50, B=3, p=0.1),
    _c("fused_n5_d64_t24_x2_half", "fusion", 64, 5, 24, 100, nb=2, B=4, p=0.5),
    _c("fused_n6_d64_gen", "block", 64, 6, 8, 64, B=5, p=0.1),             # SPW 2: 12 of 16 rows used
    _c("fused_n6_d64_t32_c1", "block", 64, 6, 32, 1, B=3),
    _c("fused_n7_d128_t24_c7", "block", 128, 7, 24, 7, B=3),                # SPW 2: 14 of 16 rows used
    _c("fused_n7_d32_t24_c33_gen", "block", 32, 7, 24, 33, B=4, p=0.1),
    _c("fused_n8_d128_c96_half", "block", 128, 8, 16, 96, B=2, p=0.5),
    _c("fused_n8_d32_c65_x8", "fusion", 32, 8, 16, 65, nb=8, B=3),
    _c("fused_lds_edge", "fusion", LDS_EDGE["D"], LDS_EDGE["N"], LDS_EDGE["T"], LDS_EDGE["C"], nb=LDS_EDGE["nb"], B=3),
    # ---- wide path (N > 8 or D > 128): per-block token launch (TM 16 for T <= 16, else 32; two samples per workgroup at
    # D = 32) + the channel-mixing launch over B*N rows ----
    _c("wide_n9_d32_t1_c33_b3", "block", 32, 9, 1, 33, B=3),                # D 32: odd B, the last workgroup holds one sample
    _c("wide_n9_d32_t8_c45_half", "block", 32, 9, 8, 45, B=5, p=0.5),
    _c("wide_n10_d32_t24_c20_half", "block", 32, 10, 24, 20, B=3, p=0.5),
    _c("wide_n11_d32_t16_c17_gen", "block", 32, 11, 16, 17, B=2, p=0.1),
    _c("wide_n12_d32_t20_c70_gen", "block", 32, 12, 20, 70, B=3, p=0.1),
    _c("wide_n127_d32_t31_c7_b5", "block", 32, 127, 31, 7, B=5),
    _c("wide_n16_d64_t5_c100", "block", 64, 16, 5, 100, B=2),
    _c("wide_n16_d64_t8_c90_gen", "block", 64, 16, 8, 90, B=3, p=0.1),
    _c("wide_n20_d64_t32_c40_gen", "block", 64, 20, 32, 40, B=2, p=0.1),
    _c("wide_n24_d64_t16_c50_half", "block", 64, 24, 16, 50, B=3, p=0.5),
    _c("wide_n33_d64_t20_c33_half", "block", 64, 33, 20, 33, B=2, p=0.5),
    _c("wide_n128_d64_t32_c65_x2", "fusion", 64, 128, 32, 65, nb=2, B=2),
    _c("wide_n17_d128_t16_c64", "block", 128, 17, 16, 64, B=3),
    _c("wide_n9_d128_t32_c100", "block", 128, 9, 32, 100, B=2),
    _c("wide_n15_d128_t8_c60_half", "block", 128, 15, 8, 60, B=2, p=0.5),
    _c("wide_n13_d128_t17_c50_half", "block", 128, 13, 17, 50, B=2, p=0.5),
    _c("wide_n18_d128_t12_c35_gen", "block", 128, 18, 12, 35, B=2, p=0.1),
    _c("wide_n100_d128_t32_c80_gen", "block", 128, 100, 32, 80, B=2, p=0.1),
    _c("wide_n33_d256_t17_c31", "block", 256, 33, 17, 31, B=2),
    _c("wide_n4_d256_t12_c40", "block", 256, 4, 12, 40, B=3),               # D 256 with N <= 8 takes the wide path
    _c("wide_n8_d256_t32_c1_b1_half", "block", 256, 8, 32, 1, B=1, p=0.5),
    _c("wide_n2_d256_t16_c70_half", "block", 256, 2, 16, 70, B=2, p=0.5),
    _c("wide_n40_d256_t8_c20_gen", "block", 256, 40, 8, 20, B=2, p=0.1),
    _c("wide_n5_d256_t24_c33_gen", "block", 256, 5, 24, 33, B=3, p=0.1),
    # ---- patch / Linear embeddings (k-block: 16 in fp32, 32 in bf16; Kp <= 3968) in front of a tower ----
    _c("embed_cin1_k49_d32", "mixer", 32, 16, 8, 40, B=3, emb=(1, (28, 28), 7)),
    _c("embed_cin3_rect_image_d64", "mixer", 64, 15, 16, 64, nb=2, B=2, emb=(3, (24, 40), 8)),
    _c("embed_cin3_k108_d32", "mixer", 32, 4, 16, 33, B=3, emb=(3, (12, 12), 6)),
    _c("embed_kp3968_d64", "mixer", 64, 4, 8, 32, B=2, emb=(62, (16, 16), 8)),
    _c("embed_k289_d256", "mixer", 256, 2, 16, 40, B=3, emb=(1, (34, 17), 17)),      # K = 288 + 1 in both precisions
    _c("embed_nopatch_k33_d128", "nopatch", 128, 6, 8, 64, nb=2, B=3, emb=33),     # (1, 33) patches: K = 32 + 1
    # ---- the MLP (exact fp32 VALU in both precisions; widths 1..128, 1..4 Linear layers) ----
    _c("mlp_w1_to_17_one_layer", "mlp", B=37, mlp=(1, 17, 1, None)),
    _c("mlp_w17_128_to_1_four_layers", "mlp", B=5, mlp=(17, 128, 3, 1)),
    _c("mlp_w128_1_four_layers", "mlp", B=9, mlp=(128, 1, 4, None)),
    _c("mlp_w128_one_layer", "mlp", B=3, mlp=(128, 128, 1, None)),
]
