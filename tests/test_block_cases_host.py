"""CPU checks behind tests/test_gpu_blocks.py: the graph walker of tests/graph_ref.py against the hand-written oracle on
the real networks, every case of tests/block_cases.py on the branch of engine.py it names (lowered without a GPU), and
every case well conditioned in float32."""
import numpy as np
import pytest
import torch

from oracle import dl3_oracle as O
from tests import block_cases as BC
from tests import graph_ref
from tests.graph_ref import l2


# ---------------------------------------------------------------------------------------------------- walker check
@pytest.mark.parametrize("backbone,head", [("mobilenetv2", "deeplab"), ("mobilenetv2", "original"),
                                           ("mobilenetv2", "subpixel"), ("xception", "deeplab")])
def test_walker_equals_the_oracle_on_the_real_graphs(backbone, head):
    """graph_ref in float64 on Deeplabv3 / SegModel graphs at 64x64 against oracle.dl3_oracle.train_grads in float64:
    logits, loss, every gradient (batch and frozen BatchNorm) and the new moving statistics, to float64 rounding — the two
    share no code beyond numpy/torch (the walker takes its operators from oracle/torch_ref.py)."""
    import dl3_amd  # noqa: F401
    from dl3_amd import graph as G
    from dl3_amd.deeplabv3p import Deeplabv3
    from dl3_amd.utils import SegModel
    shape, classes, B = (64, 64, 3), 3, 2
    G.clear_session()
    if head == "deeplab":
        model = Deeplabv3(weights=None, input_shape=shape, classes=classes, backbone=backbone, OS=16)
    else:
        model = SegModel(image_size=shape[:2]).create_seg_model(head, n=classes, backbone=backbone)
    kw = dict(backbone=backbone, input_shape=shape, classes=classes, OS=16, head=head)
    params = O.init_params(O.param_shapes(backbone, classes, head=head), seed=1)
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (B,) + shape).astype(np.float32)
    params = O.calibrate_bn(params, x, **kw)
    names = set()
    for l in model.layers:
        if l.weights:
            l.set_weights([params[n] for n in l.weights])
            names.update(l.weights)
    assert names == set(params)
    labels = rng.integers(0, classes + 1, (B, shape[0] * shape[1])).astype(np.float32)
    sw = ((labels < classes) * rng.uniform(0.5, 2.0, labels.shape)).astype(np.float32)
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    for frozen in (False, True):
        loss, grads, logits, net = O.train_grads(p64, x.astype(np.float64), labels.astype(np.float64),
                                                  sw.astype(np.float64), bn_frozen=frozen, **kw)
        r = graph_ref.run(model, x, labels, sw, dtype=torch.float64, bn_mode="frozen" if frozen else "batch")
        assert abs(r.loss - loss) < 1e-12 * abs(loss)
        assert l2(r.logits, logits) < 1e-11
        checked = 0
        for n, g in grads.items():
            if "/moving_" in n:
                continue
            assert g is not None, n
            if np.abs(g).max() < 1e-12:     # structurally zero (a bias in front of a batch-statistics BatchNorm: none here)
                assert np.abs(r.grads[n]).max() < 1e-12, n
            else:
                assert l2(r.grads[n], g) < 1e-9, (n, l2(r.grads[n], g))
            checked += 1
        assert checked == len(r.grads) == len([n for n in params if "/moving_" not in n])
        if frozen:
            assert not r.new_stats
        else:
            assert set(r.new_stats) == set(net.new_stats)
            for n, st in net.new_stats.items():
                assert l2(r.new_stats[n][0], st["mean"]) < 1e-12 and l2(r.new_stats[n][1], st["var"]) < 1e-12, n


# ---------------------------------------------------------------------------------------------------- branch check
def dry_engine(monkeypatch, c, with_knobs=True):
    """the case's plan lowered WITHOUT a GPU (tests/test_host.py::_dry_engine's method: torch.cuda.is_available patched,
    buffers on the CPU)"""
    import dl3_amd  # noqa: F401
    from dl3_amd import capi
    from dl3_amd.engine import Engine
    capi.lib()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    apply_knobs(monkeypatch, c if with_knobs else c._replace(env={}, patch=None))
    kw = BC.engine_kw(c)
    kw.pop("use_graph")
    return Engine(BC.build(c), batch=c.B, training=True, device="cpu", use_graph=False, **kw)


KNOBS = ("DL3_DY_MAT", "DL3_FUSED_ROWS", "DL3_FUSED_BWD", "DL3_FORK", "DL3_FUSE_SHUFFLE", "DL3_PRUNE_BWD", "DL3_BATCH_FOLDS",
         "DL3_POISON_SCRATCH")


def apply_knobs(monkeypatch, c):
    """the environment knobs a case names (every other knob of the lowering at its default) and its patch"""
    from dl3_amd.engine import Engine
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in c.env.items():
        assert k in KNOBS, k
        monkeypatch.setenv(k, v)
    if c.patch == "no_fold":
        # Engine.fold_tail has no knob: the engine sets it in its constructor and reads it while lowering the loss
        lower = Engine._lower_backward

        def unfolded(self):
            self.fold_tail = False
            return lower(self)
        monkeypatch.setattr(Engine, "_lower_backward", unfolded)
    else:
        assert c.patch is None, c.patch


@pytest.mark.parametrize("c", BC.RUNNABLE, ids=lambda c: c.name)
def test_case_lowers_on_its_branch(monkeypatch, c):
    e = dry_engine(monkeypatch, c)
    assert c.pred(e), (c.name, c.branches, BC.names(e.ops_fwd), BC.names(e.ops_bwd), BC.names(e.ops_prep))
    for b in e.bufs:    # (the engine's own accounting, restated: every gradient buffer got all its contributions)
        assert not (b.requires_grad and b.expected) or b.done == b.expected, b.name


@pytest.mark.parametrize("c", [c for c in BC.RUNNABLE if c.env or c.patch], ids=lambda c: c.name)
def test_predicate_fails_without_the_knob(monkeypatch, c):
    """a predicate is true ONLY on its branch: the same graph lowered with the knob at its default leaves it"""
    assert not c.pred(dry_engine(monkeypatch, c, with_knobs=False))


@pytest.mark.parametrize("c", [c for c in BC.CASES if c.raises], ids=lambda c: c.name)
def test_refused_graphs_are_refused(monkeypatch, c):
    with pytest.raises(NotImplementedError, match=c.raises):
        dry_engine(monkeypatch, c)


# the issue's list, by the names tests/block_cases.py gives the branches, plus what reading engine.py added
LISTED = """
ir.zeropad_valid_depthwise ir.dy_mat_single_tensor ir.dy_mat_off_two_tensor
res.addend_parked_then_taken res.add_gradient_aliased res.prestat_through_add res.add_feeds_add
fused.residual_addend fused.sums_against_other_tensor fused.sup1_wide_k fork.turns_dy_and_fused_off
xc.subsample_shortcut xc.sepconv_depth_activation_on xc.sepconv_depth_activation_off
xc.sum_skip_depthwise_sx xc.sum_skip_gather_grad_finish
aspp.gap aspp.rows_gemm_bn_direct aspp.resize_from_1x1_materialised aspp.rate_exceeds_map aspp.bn_at_concat_offsets
aspp.img_add_bn_path aspp.img_add_plain_path aspp.dropout_mask
dec.resize_into_slice_offset dec.resize_plain_backward dec.resize_backward_through_tmp dec.resize_source_holds_gradient
dec.skip_projection_slice
head.bilinear_folded head.bilinear_unfolded head.shuffle_loss_head head.shuffle_not_head head.plain
stem.direct_3_to_32_stride2 stem.mfma_32_to_64_sink_into_bn_act
frozen.centred_1x1 frozen.split_concat_img_unit_offset frozen.gamma_beta_only
prune.below_cut prune.bias_arm_on_pruned_input
pad.residual_odd_widths pad.concat_odd_widths pad.728_stored_736
odd.residual_b3 odd.aspp_b3
refuse.elementwise_into_slice refuse.bn_stats_through_slice refuse.resize_foreign_addend
""".split()
FOUND = """
extra.bn_epilogue_stats_above_4096_rows extra.relu_of_relu_view extra.grad_finish_alias_without_prestat
aspp.img_add_from_materialised_dy refuse.partial_first_contribution refuse.depthwise_width_not_multiple_of_4
""".split()


def test_every_branch_is_claimed():
    assert sorted(BC.BRANCHES) == sorted(LISTED + FOUND)
    claimed = {b for c in BC.CASES for b in c.branches}
    assert claimed == set(BC.BRANCHES), (sorted(set(BC.BRANCHES) - claimed), sorted(claimed - set(BC.BRANCHES)))
    assert len({c.name for c in BC.CASES}) == len(BC.CASES)
    for c in BC.CASES:
        assert c.branches and (c.pred is None) == (c.raises is not None), c.name


# ---------------------------------------------------------------------------------------------------- conditioning
COND = 5e-5


@pytest.mark.parametrize("c", BC.RUNNABLE, ids=lambda c: c.name)
def test_case_is_well_conditioned(c):
    """the float32 run of the reference lies within 5e-5 relative L2 of its float64 run on every gradient tensor (and
    1e-5 on the logits): what the device is allowed in tests/test_gpu_blocks.py is set by fp32 rounding, not by the case"""
    model, data, r64, r32 = BC.prepared(c)
    assert l2(r32.logits, r64.logits) < 1e-5
    assert abs(r32.loss - r64.loss) < 1e-5 * abs(r64.loss)
    worst = (0.0, None)
    for n, g in r64.grads.items():
        if np.abs(g).max() < 1e-12:
            continue
        worst = max(worst, (l2(r32.grads[n], g), n))
    print("%-24s seed %d worst fp32 distance %.2e (%s)" % (c.name, BC.seed_of(c), worst[0], worst[1]))
    assert worst[0] < COND, worst
