"""The configuration envelope of the fused training engines: one plain table of cases, each chosen for the dispatch decisions
(`expect`) it forces in engine.py / runtime.py / the library's host code.  Every case reaches its arm through the config dict
and the batch size alone, as a user editing patch_size / num_mixers / token_dim / num_classes in a YAML would.

tests/test_host_engine_cases.py (CPU) checks the table (both values of every decision occur, the float64 reference runs on
every config, an un-updated parameter set would show in the step-2 logits); tests/test_gpu_engine_envelope.py builds every
engine in fp32 and bf16, asserts `expect` against the built engine and compares two training steps and an evaluation with
the float64 reference.

Fields:
  name     test id
  engine   "avmnist" | "mmimdb" | "mimic"
  cfg      the complete config dict the engine is built from
  B, p     batch size, dropout (0.5: the kernels' one-bit masks, any other p > 0: 16-bit draws); the static MLP of a MIMIC case
           has no mask probe: its masks come from the host replica of the dropout stream (engine_ref.mlp_masks)
  expect   decision -> value, or -> {"fp32": value, "bf16": value} where the precisions differ (the weight-gradient launch
           covers 64 hidden columns per workgroup in fp32, 128 in bf16 below hidden_dim 128, 160 in bf16 at hidden_dim 128;
           the small-gradient slots and the single-owner embedding gradients exist in bf16 only)

Decisions (engine_ref.decisions reads them off a built engine):
  grouped, embeds_grouped      can_group(t_a, t_b, B), can_group_embeds(e_a, e_b)
  wide_a, wide_b, wide_fus     the tower takes the wide path (N > 8 or D > 128)
  heads_pool                   the heads kernel pools the towers' tokens itself
  head_part                    the heads' weight gradients go through per-workgroup slots (K * D + K + 2 <= 1472)
  fused_heads                  heads inside the fusion backward launch
  embed_fast, embed_overwrite  single-owner embedding gradients; written with "=" and kept out of Adam's clearing
  overwrite_*, groups_*, slot_*   per tower: wgrad_flags & 1, wgrad_groups(B), membership in _slot_towers
  group_slots                  wgrad_flags & 4 on the modality towers
  pack_all, adam_pack          can_pack_all, _adam_pack_modules() is not None
  time_wide, mlp_ride          MIMIC: the time tower's path, the static MLP riding in a token-mixing launch

Two decisions have one reachable value and are exempt from the both-values check (FIXED_DECISIONS): `fused_heads` is true only
under M2M_FUSED_HEADS=1 (an environment switch), and `embeds_grouped` is true by construction (the engines refuse towers of
different hidden_dim and build both embeddings in the engine's precision).

Row plans (csrc/tower_wgrad.hip wgrad_plan): a tower's rows are cut into 32-row tiles (fused path: ceil(B / (16 // N)) chain
tiles of 16 rows; wide: ceil(B N / 16)); groups = ceil(tiles / max(4, ceil(tiles / want))) with want >= ceil(32 / (slices x
blocks)), slices = ceil(Cp / columns per workgroup).  With one slice and one block: 1 group up to 4 tiles, 2 groups for 5..8,
3 for 9..12.
"""
from collections import namedtuple

Case = namedtuple("Case", "name engine cfg B p expect")

DECISIONS = ("grouped", "embeds_grouped", "wide_a", "wide_b", "wide_fus", "heads_pool", "head_part", "fused_heads", "embed_fast",
             "embed_overwrite", "overwrite_a", "overwrite_b", "overwrite_fus", "groups_a", "groups_b", "groups_fus",
             "slot_a", "slot_b", "slot_fus", "group_slots", "pack_all", "adam_pack", "time_wide", "mlp_ride")
FIXED_DECISIONS = {"fused_heads": False, "embeds_grouped": True}

BY_PREC = lambda fp32, bf16: {"fp32": fp32, "bf16": bf16}


def _tower(D, image, patch, T=16, C=33, nb=1, cin=1):
    return dict(in_channels=cin, hidden_dim=D, patch_size=patch, image_size=list(image), token_dim=T, channel_dim=C, num_mixers=nb)


def _fusion(D, T=16, C=33, nb=1):
    return dict(hidden_dim=D, token_dim=T, channel_dim=C, num_mixers=nb)


def _av(name, image, audio, fusion, B=13, p=0.0, K=10, **expect):
    return Case(name, "avmnist", dict(dropout=p, num_classes=K, image=image, audio=audio, multimodal=fusion), B, p, expect)


def _mm(name, image, text, fusion, B=5, p=0.0, K=5, **expect):
    cfg = dict(dropout=p, num_classes=K, image=image, text=text, multimodal=fusion, pos_weight=[1.5 + 2.0 * i for i in range(K)])
    return Case(name, "mmimdb", cfg, B, p, expect)


def _mimic(name, num_patch, B=13, D=64, p=0.0, time_mixers=1, **expect):
    cfg = dict(dropout=p, num_classes=6,
               time=dict(embedding_dim=12, proj_dim=D, hidden_dim=D, num_patch=num_patch, token_dim=16, channel_dim=33, num_mixers=time_mixers),
               static=dict(input_dim=5, hidden_dim=24, num_blocks=2, output_dim=D),
               multimodal=dict(hidden_dim=D, token_dim=8, channel_dim=100, num_mixers=1))
    return Case(name, "mimic", cfg, B, p, expect)


# token counts from small images: (4, 4) / 4 -> 1, (8, 4) / 4 -> 2, (12, 4) / 4 -> 3, (8, 8) / 4 -> 4, (8, 12) / 4 -> 6,
# (16, 16) / 4 -> 16; the second modality uses another patch size (8) where the count allows it
CASES = [
    # ---- AV-MNIST engine ------------------------------------------------------------------------------------------------
    # the grouped launches with Na != Nb: SPW 8 beside SPW 4, fusion N = 6 (SPW 2, 12 of 16 rows used)
    _av("av_grouped_n2_n4_d64_half", _tower(64, (8, 4), 4, T=16, C=33), _tower(64, (16, 16), 8, T=16, C=100), _fusion(64, T=24, C=33),
        p=0.5, grouped=True, wide_a=False, wide_b=False, wide_fus=False, heads_pool=False, head_part=True, fused_heads=False,
        embeds_grouped=True, embed_fast=BY_PREC(False, True), embed_overwrite=BY_PREC(False, True), group_slots=False,
        overwrite_a=True, overwrite_b=True, overwrite_fus=True, groups_a=1, groups_b=1, groups_fus=1,
        slot_a=False, slot_b=False, slot_fus=False, pack_all=True, adam_pack=True),
    # N = 1 beside N = 3 (SPW 16 and 5: 15 of 16 rows used), fusion N = 4; hidden_dim 128: bf16 collects the pair's small gradients
    # in per-workgroup slots
    _av("av_grouped_n1_n3_d128_gen", _tower(128, (4, 4), 4, T=24, C=33), _tower(128, (12, 4), 4, T=24, C=100, cin=2),
        _fusion(128, T=8, C=33, nb=2), p=0.1, grouped=True, group_slots=BY_PREC(False, True), wide_fus=False, head_part=True,
        embed_fast=BY_PREC(False, True), embed_overwrite=BY_PREC(False, True)),
    # token counts on both sides of N <= 4: two streams, single-tower launches; wide fusion tower (N = 10) over fused towers; in
    # bf16 both towers have small-gradient slots but the pair's launch does not exist
    _av("av_token_class_n4_n6_d128_half", _tower(128, (8, 8), 4, T=16, C=33), _tower(128, (8, 12), 4, T=16, C=100), _fusion(128, T=16, C=33),
        p=0.5, grouped=False, group_slots=False, wide_a=False, wide_b=False, wide_fus=True, heads_pool=False, head_part=True,
        embed_fast=BY_PREC(False, True)),
    # token_dim 16 beside 8: different token-mixing builds
    _av("av_token_dim_16_8_d32", _tower(32, (8, 8), 4, T=16, C=33), _tower(32, (16, 16), 8, T=8, C=33), _fusion(32, T=16, C=100),
        grouped=False, wide_a=False, wide_b=False, wide_fus=False, pack_all=True, adam_pack=True),
    # a fused tower beside a wide one, wide fusion tower: the fused tower pools in its chain launch, the wide ones append the
    # token-mean launch, the heads do not pool
    _av("av_fused_n4_wide_n16_d64_gen", _tower(64, (8, 8), 4, T=16, C=33), _tower(64, (16, 16), 4, T=16, C=100), _fusion(64, T=24, C=33),
        p=0.1, grouped=False, wide_a=False, wide_b=True, wide_fus=True, heads_pool=False, embed_fast=False, embed_overwrite=False),
    # all three towers wide at hidden_dim 64: not a wide pair (that needs 256), cross-entropy heads pooling the tokens themselves
    _av("av_all_wide_n16_n16_d64", _tower(64, (16, 16), 4, T=16, C=33), _tower(64, (32, 32), 8, T=8, C=33), _fusion(64, T=16, C=33),
        B=5, grouped=False, wide_a=True, wide_b=True, wide_fus=True, heads_pool=True, head_part=True, embed_fast=False),
    # five blocks in one tower: no pair launch, per-module pack, Adam and the re-pack as two launches
    _av("av_five_blocks_d32", _tower(32, (8, 8), 4, T=16, C=33, nb=5), _tower(32, (16, 16), 8, T=16, C=33), _fusion(32, T=16, C=33),
        grouped=False, pack_all=False, adam_pack=False, overwrite_a=True, overwrite_b=True, overwrite_fus=True),
    # 4 + 4 + 8 blocks: the towers' ranges fill the table of 16 exactly, the embeddings' two do not fit
    _av("av_ranges_full_4_4_8_d32", _tower(32, (8, 8), 4, T=16, C=33, nb=4), _tower(32, (16, 16), 8, T=16, C=33, nb=4),
        _fusion(32, T=16, C=33, nb=8), grouped=True, embed_fast=BY_PREC(False, True), embed_overwrite=False,
        overwrite_a=True, overwrite_b=True, overwrite_fus=True, pack_all=False, adam_pack=False),
    # 4 + 5 + 8 blocks: 17 ranges, the audio tower (last in the launch) is left accumulating and Adam clears it; the 12 ranges
    # that remain leave room for the embeddings' two
    _av("av_ranges_over_4_5_8_d32", _tower(32, (8, 8), 4, T=16, C=33, nb=4), _tower(32, (16, 16), 8, T=16, C=33, nb=5),
        _fusion(32, T=16, C=33, nb=8), grouped=False, overwrite_a=True, overwrite_b=False, overwrite_fus=True,
        embed_overwrite=BY_PREC(False, True), pack_all=False),
    # K = 12 at hidden_dim 128: 12 * 128 + 12 + 2 > 1472, the heads add their weight gradients with float atomics
    _av("av_classes_12_d128", _tower(128, (8, 8), 4, T=16, C=33), _tower(128, (16, 16), 8, T=16, C=33), _fusion(128, T=16, C=33),
        K=12, grouped=True, head_part=False, fused_heads=False, group_slots=BY_PREC(False, True)),
    # B = 19: the fusion tower (N = 8: 10 chain tiles, 5 streamed tiles) has two row groups, the modality towers (N = 4: 3
    # streamed tiles) one -- the second group goes through the slot that Adam (or forward_backward's fold) adds
    _av("av_fusion_two_groups_b19_d32_gen", _tower(32, (8, 8), 4, T=16, C=33), _tower(32, (16, 16), 8, T=16, C=33), _fusion(32, T=16, C=33),
        B=19, p=0.3, grouped=True, groups_a=1, groups_b=1, groups_fus=2, slot_a=False, slot_b=False, slot_fus=True,
        overwrite_a=True, overwrite_b=True, overwrite_fus=True),
    # B = 33: the fusion tower has 9 streamed tiles -> three row groups: no overwrite, float atomics, Adam clears its ranges;
    # the modality towers (5 tiles) have two groups and take slots
    _av("av_fusion_three_groups_b33_d32", _tower(32, (8, 8), 4, T=16, C=33), _tower(32, (16, 16), 8, T=16, C=33), _fusion(32, T=16, C=33),
        B=33, grouped=True, groups_a=2, groups_b=2, groups_fus=3, slot_a=True, slot_b=True, slot_fus=False,
        overwrite_a=True, overwrite_b=True, overwrite_fus=False),
    # B = 70: every tower has three or more row groups (9, 9 and 18 streamed tiles): nothing overwrites, only the embeddings'
    # ranges are kept
    _av("av_all_towers_many_groups_b70_d32_half", _tower(32, (8, 8), 4, T=16, C=33), _tower(32, (16, 16), 8, T=16, C=33), _fusion(32, T=16, C=33),
        B=70, p=0.5, grouped=True, groups_a=3, groups_b=3, groups_fus=5, slot_a=False, slot_b=False, slot_fus=False,
        overwrite_a=False, overwrite_b=False, overwrite_fus=False, embed_overwrite=BY_PREC(False, True)),
    # four blocks x channel_dim 256 at B = 46 (fusion N = 8: 12 streamed tiles): fp32 has 4 column slices -> 16 workgroups per
    # row group, want = 2 -> two groups (slot); bf16 has 2 slices -> want = 4 -> three groups (atomics)
    _av("av_row_plan_by_precision_b46_d64", _tower(64, (8, 8), 4, T=16, C=33), _tower(64, (16, 16), 8, T=16, C=33),
        _fusion(64, T=16, C=256, nb=4), B=46, grouped=True, groups_fus=BY_PREC(2, 3), slot_fus=BY_PREC(True, False),
        overwrite_fus=BY_PREC(True, False)),
    # ---- MM-IMDb engine (hidden_dim 256: every tower wide, BCE heads) ------------------------------------------------------
    # the wide pair's launches with Na = 6 beside Nb = 15
    _mm("mm_wide_pair_n6_n15_half", _tower(256, (8, 12), 4, T=16, C=33, cin=3), _tower(256, (12, 20), 4, T=8, C=100), _fusion(256, T=16, C=33),
        p=0.5, grouped=True, wide_a=True, wide_b=True, wide_fus=True, heads_pool=True, head_part=False, embed_fast=False,
        embed_overwrite=False, group_slots=False),
    # token_dim 32: refused by the pair launch (16 waves per workgroup hold token_dim <= 16)
    _mm("mm_token_dim_32", _tower(256, (8, 12), 4, T=32, C=33, cin=3), _tower(256, (8, 8), 4, T=32, C=33), _fusion(256, T=16, C=33),
        grouped=False, heads_pool=True),
    # unequal block counts: refused by the pair launch
    _mm("mm_mixers_1_2_gen", _tower(256, (8, 12), 4, T=16, C=33, cin=3), _tower(256, (8, 8), 4, T=16, C=33, nb=2), _fusion(256, T=16, C=33),
        p=0.1, grouped=False, heads_pool=True, pack_all=True, adam_pack=True),
    # ---- MIMIC engine: fused time tower (num_patch <= 8): the heads pool a fused tower's strided tokens, the riding MLP has no
    # carrier and is launched by ride_flush ---------------------------------------------------------------------------------
    _mimic("mimic_patches_7", 7, time_wide=False, wide_fus=False, heads_pool=True, mlp_ride=True),
    _mimic("mimic_patches_8", 8, time_wide=False, wide_fus=True, heads_pool=True, mlp_ride=True),
    # past batch 2048 the MLP has launches of its own and the step runs on three streams with per-segment Adam
    _mimic("mimic_patches_9_b2049", 9, B=2049, D=32, time_wide=True, wide_fus=True, mlp_ride=False),
    # dropout on: the static MLP's masks are the host replica's.  The flushed ride under the one-bit and the 16-bit stream ...
    _mimic("mimic_patches_7_half", 7, p=0.5, time_wide=False, wide_fus=False, heads_pool=True, mlp_ride=True),
    _mimic("mimic_patches_8_gen", 8, p=0.1, time_wide=False, wide_fus=True, heads_pool=True, mlp_ride=True),
    # ... and the MLP riding in a wide time tower's token-mixing launch (the carrier draws masks of its own in the same launch).
    # Two time blocks: with one, hidden_dim 32 at batch 13 has too few parameters for the stale-parameter condition of
    # tests/test_host_engine_cases.py (step-2 logits move by 0.125 < 10 x the bf16 bar; 0.232 with two)
    _mimic("mimic_patches_9_wide_carrier_half", 9, D=32, p=0.5, time_mixers=2, time_wide=True, wide_fus=True, heads_pool=True, mlp_ride=True),
    # past batch 2048 with dropout: the MLP's own launches (VALU kernels) beside the towers on three streams
    _mimic("mimic_patches_9_b2049_gen", 9, B=2049, D=32, p=0.3, time_wide=True, wide_fus=True, mlp_ride=False),
]
