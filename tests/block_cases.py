"""Small graphs, one per branch of the engine's backward wiring (engine.py: contrib_kernel / contrib_passthrough /
contrib_elementwise, alias_stats_target, prestat, finish_bn_bwd, grad_operand, GradSink and the units' bwd()).

Shared by tests/test_block_cases_host.py (every case lowers on a dry engine and sits on the branch it names; its float32
reference run is well conditioned) and tests/test_gpu_blocks.py (one step on the device against tests/graph_ref.py in
float64).  A case: name, builder over the graph API, batch, input shape, Engine keywords, environment knobs, the branches
it exists for and a predicate over the lowered plan that holds only when those branches were taken.  Shapes are the
smallest that keep >= ~500 rows per BatchNorm channel: fp32 rounding, not depth, sets the error bar."""
import collections

import numpy as np

CLASSES = 3

# every branch of the wiring a case must claim (tests/test_block_cases_host.py::test_every_branch_is_claimed)
BRANCHES = (
    # inverted-residual block, no skip, stride 2
    "ir.zeropad_valid_depthwise", "ir.dy_mat_single_tensor", "ir.dy_mat_off_two_tensor",
    # ... with the residual Add
    "res.addend_parked_then_taken", "res.add_gradient_aliased", "res.prestat_through_add", "res.add_feeds_add",
    # DL3_FUSED_ROWS=1 / DL3_FORK=1
    "fused.residual_addend", "fused.sums_against_other_tensor", "fused.sup1_wide_k", "fork.turns_dy_and_fused_off",
    # Xception blocks
    "xc.subsample_shortcut", "xc.sepconv_depth_activation_on", "xc.sepconv_depth_activation_off",
    "xc.sum_skip_depthwise_sx", "xc.sum_skip_gather_grad_finish",
    # ASPP
    "aspp.gap", "aspp.rows_gemm_bn_direct", "aspp.resize_from_1x1_materialised", "aspp.rate_exceeds_map",
    "aspp.bn_at_concat_offsets", "aspp.img_add_bn_path", "aspp.img_add_plain_path", "aspp.dropout_mask",
    # decoder
    "dec.resize_into_slice_offset", "dec.resize_plain_backward", "dec.resize_backward_through_tmp",
    "dec.resize_source_holds_gradient", "dec.skip_projection_slice",
    # heads
    "head.bilinear_folded", "head.bilinear_unfolded", "head.shuffle_loss_head", "head.shuffle_not_head", "head.plain",
    # stems
    "stem.direct_3_to_32_stride2", "stem.mfma_32_to_64_sink_into_bn_act",
    # frozen BatchNorm
    "frozen.centred_1x1", "frozen.split_concat_img_unit_offset", "frozen.gamma_beta_only",
    # pruned gradients
    "prune.below_cut", "prune.bias_arm_on_pruned_input",
    # stored-channel padding
    "pad.residual_odd_widths", "pad.concat_odd_widths", "pad.728_stored_736",
    # odd batch
    "odd.residual_b3", "odd.aspp_b3",
    # found while reading engine.py (not in the issue's list)
    "extra.bn_epilogue_stats_above_4096_rows", "extra.relu_of_relu_view", "extra.grad_finish_alias_without_prestat",
    "aspp.img_add_from_materialised_dy",
    # refusals
    "refuse.elementwise_into_slice", "refuse.bn_stats_through_slice", "refuse.resize_foreign_addend",
    "refuse.partial_first_contribution", "refuse.depthwise_width_not_multiple_of_4",
)

Case = collections.namedtuple("Case", "name build B shape kw env patch branches pred raises seeds")


def case(name, build, B, shape, branches, pred, kw=None, env=None, patch=None, raises=None, seeds=(1, 2, 3, 4, 5, 6)):
    return Case(name, build, B, shape, dict(kw or {}), dict(env or {}), patch, tuple(branches), pred, raises, seeds)


# ---------------------------------------------------------------------------------------------------- builders
def _bn(G, x, name, eps=1e-3, momentum=0.99):
    return G.BatchNormalization(name=name, epsilon=eps, momentum=momentum)(x)


def _cbr(G, x, n, name, act="relu", eps=1e-3):
    """1x1 convolution -> BatchNorm [-> activation]"""
    x = _bn(G, G.Conv2D(n, 1, padding="same", use_bias=False, name=name)(x), name + "_BN", eps)
    return G.Activation(act, name=name + "_act")(x) if act else x


def _finish(G, inp, x, head="plain", size=None, r=2, name="blk"):
    """the logits convolution and one of the three heads; size: the (H, W) the labels live at"""
    if head == "plain":
        x = G.Conv2D(CLASSES, 1, padding="same", name="logits")(x)
    elif head == "bilinear":
        x = G.Conv2D(CLASSES, 1, padding="same", name="logits")(x)
        x = G.ResizeBilinear(size, name="up")(x)
    else:
        from dl3_amd.subpixel import Subpixel
        x = Subpixel(CLASSES, 1, r, name="logits")(x)
    H, W = x.shape[0], x.shape[1]
    x = G.Reshape((H * W, -1))(x)
    x = G.Activation("softmax", name="pred_mask")(x)
    return G.Model(inp, x, name=name)


def _ir_block(G, x, prefix, expand, filters, stride=1, skip=False, zeropad=False, rate=1):
    """MobileNetV2 inverted residual: expand 1x1 -> BN -> relu6 -> depthwise -> BN -> relu6 -> project 1x1 -> BN [+ input]"""
    inp = x
    x = _cbr(G, x, expand, prefix + "expand", "relu6")
    padding = "same"
    if zeropad:
        x = G.ZeroPadding2D((1, 1), name=prefix + "pad")(x)
        padding = "valid"
    x = G.DepthwiseConv2D(3, strides=stride, padding=padding, use_bias=False, dilation_rate=(rate, rate),
                          name=prefix + "depthwise")(x)
    x = G.Activation("relu6", name=prefix + "depthwise_act")(_bn(G, x, prefix + "depthwise_BN"))
    x = _cbr(G, x, filters, prefix + "project", None)
    return G.Add(name=prefix + "add")([inp, x]) if skip else x


def _sepconv(G, x, filters, prefix, stride=1, rate=1, depth_activation=False, eps=1e-3):
    padding = "same"
    if stride != 1:
        x = G.ZeroPadding2D((1, 1), name=prefix + "_pad")(x)
        padding = "valid"
    if not depth_activation:
        x = G.Activation("relu", name=prefix + "_pre")(x)
    x = G.DepthwiseConv2D(3, strides=stride, dilation_rate=(rate, rate), padding=padding, use_bias=False,
                          name=prefix + "_depthwise")(x)
    x = _bn(G, x, prefix + "_depthwise_BN", eps)
    if depth_activation:
        x = G.Activation("relu", name=prefix + "_dact")(x)
    x = _bn(G, G.Conv2D(filters, 1, padding="same", use_bias=False, name=prefix + "_pointwise")(x), prefix + "_pointwise_BN", eps)
    if depth_activation:
        x = G.Activation("relu", name=prefix + "_pact")(x)
    return x


def ir_noskip(G, shape):
    inp = G.Input(shape=shape)
    x = _cbr(G, inp, 16, "stem", None)
    x = _ir_block(G, x, "b1_", 48, 24, stride=2, zeropad=True)
    return _finish(G, inp, x)


def ir_res(widths=(16, 48), blocks=1, stem_act=None):
    def build(G, shape):
        inp = G.Input(shape=shape)
        x = _cbr(G, inp, widths[0], "stem", stem_act)
        for i in range(blocks):
            x = _ir_block(G, x, "b%d_" % (i + 1), widths[1], widths[0], skip=True)
        return _finish(G, inp, x)
    return build


def ir_wide(G, shape):
    """a project convolution with K = 96 > 64 (dl3_pwconv_bwd_fused_supported == 1) between two residual blocks' tensors"""
    inp = G.Input(shape=shape)
    x = _cbr(G, inp, 16, "stem", None)
    x = _ir_block(G, x, "b1_", 96, 16, skip=True)
    return _finish(G, inp, x)


def xc_conv_shortcut(G, shape):
    inp = G.Input(shape=shape)
    x = _cbr(G, inp, 16, "stem", "relu")
    r = _sepconv(G, x, 24, "s1")
    r = _sepconv(G, r, 24, "s2", depth_activation=True)
    r = _sepconv(G, r, 24, "s3", stride=2)
    sc = G.Conv2D(24, 1, strides=2, padding="valid", use_bias=False, name="shortcut")(x)
    sc = _bn(G, sc, "shortcut_BN")
    x = G.Add(name="add")([r, sc])
    return _finish(G, inp, x)


def xc_sum_skip(units=2):
    def build(G, shape):
        inp = G.Input(shape=shape)
        x = _cbr(G, inp, 24, "stem", None)
        for u in range(units):
            r = x
            for i in range(2):
                r = _sepconv(G, r, 24, "u%d_s%d" % (u + 1, i + 1))
            x = G.Add(name="u%d_add" % (u + 1))([r, x])
        return _finish(G, inp, x)
    return build


def aspp(first=True, proj_bn=True, dropout=True, head="plain", rates=(2, 18), widths=(32, 16, 32)):
    """feature -> [image pooling | 1x1 | atrous separable branches] -> Concatenate -> projection [-> BN -> relu -> Dropout].
    first: the pooled branch leads the Concatenate (never materialised: a per-image addend of the projection).
    Rate 18 on the 20x16 map: every horizontal tap and all but two rows of the vertical ones fall outside.  (A rate beyond
    BOTH sizes leaves the centre tap alone — a per-channel scale in front of a BatchNorm, whose gradient is zero up to
    epsilon: a tensor that is all cancellation, which no relative bound can judge.)"""
    cf, cb, cp = widths

    def build(G, shape):
        H, W = shape[0], shape[1]
        inp = G.Input(shape=shape)
        x = _cbr(G, inp, cf, "feat", "relu")
        b4 = G.AveragePooling2D(pool_size=(H, W), name="gap")(x)
        b4 = _cbr(G, b4, cb, "image_pooling", "relu", eps=1e-5)
        b4 = G.ResizeBilinear((H, W), name="pool_up")(b4)
        b0 = _cbr(G, x, cb, "aspp0", "relu", eps=1e-5)
        bs = [_sepconv(G, x, cb, "aspp%d" % (i + 1), rate=r, depth_activation=True, eps=1e-5) for i, r in enumerate(rates)]
        x = G.Concatenate(name="cat")([b4, b0] + bs if first else [b0] + bs + [b4])
        if proj_bn:
            x = _cbr(G, x, cp, "concat_projection", "relu", eps=1e-5)
        else:
            x = G.Activation("relu", name="proj_act")(G.Conv2D(cp, 1, padding="same", name="concat_projection")(x))
        if dropout:
            x = G.Dropout(0.1, name="drop")(x)
        return _finish(G, inp, x, head, size=(H, W))
    return build


def decoder(swap=False, dropout=True, twice=False):
    """low-resolution trunk -> [Dropout] -> resize x2 | skip projection -> Concatenate -> separable convolution.
    swap: the skip leads the Concatenate (the resize writes at a channel offset); twice: the trunk is resized into two
    slices, so its buffer already holds a gradient when the first resize's backward arrives"""
    def build(G, shape):
        H, W = shape[0], shape[1]
        inp = G.Input(shape=shape)
        skip = _cbr(G, inp, 16, "enc", "relu")
        t = _sepconv(G, skip, 24, "down", stride=2, depth_activation=True)
        if dropout:
            t = G.Dropout(0.1, name="drop")(t)
        up = G.ResizeBilinear((H, W), name="dec_up")(t)
        proj = _cbr(G, skip, 8, "feature_projection0", "relu", eps=1e-5)
        parts = [proj, up] if swap else [up, proj]
        if twice:
            parts.append(G.ResizeBilinear((H, W), name="dec_up2")(t))
        x = G.Concatenate(name="dec_cat")(parts)
        x = _sepconv(G, x, 16, "decoder_conv0", depth_activation=True, eps=1e-5)
        return _finish(G, inp, x)
    return build


def head_only(head, r=2):
    def build(G, shape):
        H, W = shape[0], shape[1]
        inp = G.Input(shape=shape)
        x = _cbr(G, inp, 16, "c0", "relu")
        if head == "bilinear":
            x = _sepconv(G, x, 16, "down", stride=2, depth_activation=True)
        return _finish(G, inp, x, head, size=(H, W), r=r)
    return build


def stems(G, shape):
    inp = G.Input(shape=shape)
    x = G.Prescale(name="prescale")(inp)
    x = G.Conv2D(32, 3, strides=2, padding="same", use_bias=False, name="conv1_1")(x)
    x = G.Activation("relu", name="conv1_1_act")(_bn(G, x, "conv1_1_BN"))
    x = G.Conv2D(64, 3, padding="same", use_bias=False, name="conv1_2")(x)
    x = G.Activation("relu", name="conv1_2_act")(_bn(G, x, "conv1_2_BN"))
    return _finish(G, inp, x, "bilinear", size=(shape[0], shape[1]))


def pruned(G, shape):
    """the stem and the first block are frozen (`trainable = False` before the engine is built); a biased convolution
    reads the frozen region's output.  A Conv2D's kernel and bias share their layer's flag, so `kernel frozen, bias
    trains` cannot be stated through the graph API: the bias arm of PwUnit.bwd is reached with both trainable, on an
    input that needs no gradient (the launch folds dW and db itself, and bwd() returns before its bwd-data)"""
    inp = G.Input(shape=shape)
    x = _cbr(G, inp, 16, "stem", None)
    x = _ir_block(G, x, "b1_", 48, 16, skip=True)
    x = G.Activation("relu", name="mid_act")(G.Conv2D(16, 1, padding="same", name="mid")(x))
    x = _ir_block(G, x, "b2_", 48, 16, skip=True)
    m = _finish(G, inp, x)
    for l in m.layers:
        if l.name.startswith(("stem", "b1_")):
            l.trainable = False
    return m


def wide_728(G, shape):
    inp = G.Input(shape=shape)
    x = _cbr(G, inp, 728, "wide", "relu")
    x = _sepconv(G, x, 8, "s1", depth_activation=True)
    return _finish(G, inp, x)


def relu_of_relu(G, shape):
    """Xception's entry_flow_block1: a separable convolution without depth_activation re-applies ReLU to a rectified view"""
    inp = G.Input(shape=shape)
    x = _cbr(G, inp, 16, "stem", "relu")
    x = _sepconv(G, x, 16, "s1")
    return _finish(G, inp, x)


def add_of_two_bn(G, shape):
    """Add of two BatchNorm'ed convolution outputs straight into the logits layer: both inputs qualify for the early sums,
    alias_stats_target returns none, and each aliased gradient gets its own dl3_grad_finish pass for the sums"""
    inp = G.Input(shape=shape)
    x = _cbr(G, inp, 16, "stem", "relu")
    x = G.Add(name="add")([_cbr(G, x, 16, "left", None), _cbr(G, x, 16, "right", None)])
    return _finish(G, inp, x)


def refuse_elementwise_slice(G, shape):
    H, W = shape[0], shape[1]
    inp = G.Input(shape=shape)
    x = _cbr(G, inp, 16, "feat", "relu")
    b0, b1 = _cbr(G, x, 8, "aspp0", "relu"), _cbr(G, x, 8, "aspp1", "relu")
    p = _cbr(G, G.AveragePooling2D(pool_size=(H, W), name="gap")(b0), 8, "image_pooling", "relu")
    x = G.Concatenate(name="cat")([b0, b1, G.ResizeBilinear((H, W), name="pool_up")(p)])
    return _finish(G, inp, _cbr(G, x, 16, "proj", "relu"))


def refuse_slice_consumer(side_first):
    """a tensor that lives in a Concatenate slice has a second consumer.  side_first: that consumer is lowered before the
    Concatenate's (its backward comes last and would owe the BatchNorm sums of a slice); otherwise its backward comes
    first and writes one slice of a fresh gradient buffer that the next contribution then adds to as a whole"""
    def build(G, shape):
        inp = G.Input(shape=shape)
        x = _cbr(G, inp, 16, "feat", "relu")
        b0, b1 = _cbr(G, x, 8, "aspp0", "relu"), _cbr(G, x, 8, "aspp1", "relu")
        side = _cbr(G, b0, 16, "side", None)
        x = _cbr(G, G.Concatenate(name="cat")([b0, b1]), 16, "proj", None)
        return _finish(G, inp, G.Add(name="add")([side, x] if side_first else [x, side]))
    return build


def refuse_foreign_addend(G, shape):
    H, W = shape[0], shape[1]
    inp = G.Input(shape=shape)
    x = _cbr(G, inp, 16, "feat", "relu")
    t = G.Dropout(0.1, name="drop")(x)                        # a materialised, plain tensor with two consumers
    up = G.ResizeBilinear((H, W), name="same_size")(t)
    y = _cbr(G, G.Concatenate(name="cat")([up, _cbr(G, x, 8, "other", "relu")]), 16, "proj", None)
    return _finish(G, inp, G.Add(name="add")([t, y]))         # the Add parks its gradient on t before the resize arrives


# ---------------------------------------------------------------------------------------------------- predicates
def ops(lst, name):
    """the records of entry point `name`: their arguments are read by the header's names (engine.Launch.arg)"""
    return [rec for rec in lst if rec[0] == name]


def vals(rec, *keys):
    return [rec.arg(k) for k in keys]


def names(lst):
    return [rec[0] for rec in lst]


def _buf(eng, name):
    return [b for b in eng.bufs if b.name == name][0]


def _ptr(t):
    return t.data_ptr()


def p_zeropad(e):
    d = ops(e.ops_fwd, "dl3_dwconv3x3_fwd")
    return (len(d) == 1 and vals(d[0], "stride", "rate", "pad_t", "pad_l") == [2, 1, 1, 1]
            and "dl3_dwconv3x3_bwd" in names(e.ops_bwd))


def p_dy_on(e):
    wd, bd = ops(e.ops_bwd, "dl3_pwconv_bwd_weight_dy"), ops(e.ops_bwd, "dl3_pwconv_bwd_data")
    dy = e.dy_buf is not None and _ptr(e.dy_buf)
    return bool(wd) and any(a.arg("g") == dy and a.arg("yraw") is None and a.arg("cA") is None for a in bd)


def p_dy_off(e):
    bd = ops(e.ops_bwd, "dl3_pwconv_bwd_data")
    return (e.dy_buf is None and not ops(e.ops_bwd, "dl3_pwconv_bwd_weight_dy")
            and sum(a.arg("cA") is not None for a in bd) >= 2)


def _adds(e):
    return [u for u in e.units if type(u).__name__ == "AddUnit"]


def p_residual(e):
    """the block input's first contribution was parked as addend and taken as `add` by the expand convolution's bwd-data;
    the Add's gradient is the project buffer's gradient; that buffer's sums came from a bwd-data epilogue (no
    dl3_grad_finish in the plan)"""
    ok = "dl3_grad_finish" not in names(e.ops_bwd) and not e.prestat
    for u in _adds(e):
        g = u.outv.buf.grad
        ok = ok and u.b.buf.grad is g and u.a.buf.grad is not g
        # (dl3_pwconv_bwd_data and dl3_pwconv_bwd_fused share the names of the gradient they write and its addend)
        taken = [a for a in ops(e.ops_bwd, "dl3_pwconv_bwd_data") + ops(e.ops_bwd, "dl3_pwconv_bwd_fused")
                 if a.arg("dx") == _ptr(u.a.buf.grad) and a.arg("dx_add") == _ptr(g)]
        ok = ok and len(taken) == 1
        early = [a for a in ops(e.ops_bwd, "dl3_pwconv_bwd_data")
                 if vals(a, "dx", "x_mean", "x") == [_ptr(g), u.b.buf.vptr(2), _ptr(u.b.buf.t)]]
        early += [a for a in ops(e.ops_bwd, "dl3_pwconv_bwd_fused")
                  if vals(a, "dx", "x_mean", "stat_x") == [_ptr(g), u.b.buf.vptr(2), _ptr(u.b.buf.t)]]
        ok = ok and len(early) == 1
    return ok and bool(_adds(e))


def p_stacked(e):
    adds = _adds(e)
    return len(adds) == 2 and adds[1].a.buf is adds[0].outv.buf and not adds[0].outv.buf.bns and p_residual(e)


def p_fused(e):
    f = ops(e.ops_bwd, "dl3_pwconv_bwd_fused")
    own = lambda a: a.arg("stat_x") == a.arg("x")   # noqa: E731  (sums against the forward input itself)
    return (p_residual(e) and any(a.arg("dx_add") is not None for a in f)
            and any(a.arg("x_mean") is not None and not own(a) for a in f) and len(f) >= 3)


def p_fused_sup1(e):
    wide = [a for a in ops(e.ops_bwd, "dl3_pwconv_bwd_fused") if a.arg("K") > 64]
    return len(wide) == 1 and all(
        e.lib.dl3_pwconv_bwd_fused_supported(*vals(a, "M", "K", "N")) == 1 and a.arg("dx_add") is None
        and (a.arg("x_mean") is None or a.arg("stat_x") == a.arg("x")) for a in wide)


def p_fork(e):
    n = names(e.ops_bwd)
    return e.fork and bool(e._side) and "dl3_pwconv_bwd_fused" not in n and "dl3_pwconv_bwd_weight_dy" not in n \
        and e.dy_buf is None


def p_subsample(e):
    n = names(e.ops_bwd)
    i = n.index("dl3_subsample_bwd") if "dl3_subsample_bwd" in n else -1
    d = [vals(a, "stride", "rate") for a in ops(e.ops_fwd, "dl3_dwconv3x3_fwd")]
    acts = [a.arg("in_act") for a in ops(e.ops_fwd, "dl3_dwconv3x3_fwd")]
    return ("dl3_subsample_fwd" in names(e.ops_fwd) and i >= 0 and n[i + 1] == "dl3_grad_finish" and [2, 1] in d
            and acts == [1, 0, 1])   # relu of a rectified view, none in front of depth_activation, the leading relu


def p_dw_sx(e):
    sx = ops(e.ops_bwd, "dl3_dwconv3x3_bwd_sx")
    return len(sx) == 1 and sx[0].arg("x_mean") is not None and "dl3_grad_finish" not in names(e.ops_bwd) and len(_adds(e)) == 2


def p_dw_gather(e):
    n = names(e.ops_bwd)
    return "dl3_dwconv3x3_bwd_sx" not in n and n.count("dl3_grad_finish") >= 1 and all(
        a.arg("impl") == 1 for a in ops(e.ops_bwd, "dl3_dwconv3x3_bwd"))


def _cat(e, name="cat"):
    return _buf(e, name)


def p_aspp_split(mode=None):
    """mode: how the per-image addend's gradient is summed — "bn": two coefficient-weighted column sums and their sum
    (cA given); "dy": one plain sum over the dY the weight-gradient launch materialised; "plain": one plain sum over g"""
    def pred(e):
        cat = _cat(e)
        f, b = names(e.ops_fwd), names(e.ops_bwd)
        rows = ops(e.ops_fwd, "dl3_pwconv_fwd_rows")
        add = ops(e.ops_fwd, "dl3_pwconv_fwd_add")
        gaps = ops(e.ops_bwd, "dl3_gap_fwd")
        ok = (f.count("dl3_gap_fwd") == 1 and len(rows) == 2 and len(add) == 1 and id(cat) in e.bcast_src
              and "dl3_resize_bilinear_fwd" not in f and "dl3_resize_bilinear_bwd" not in b
              and f.count("dl3_bn_finalize_direct") >= 5
              and [o for _, o, _ in cat.bns] == [0, cat.ld // 3, 2 * cat.ld // 3]
              # the second rows GEMM reads kernel row 0, the per-pixel GEMM the rows behind the pooled branch's
              and add[0].arg("w") - rows[1].arg("w") == 4 * rows[1].arg("K") * rows[1].arg("N"))
        big = [a for a in ops(e.ops_fwd, "dl3_dwconv3x3_fwd") if a.arg("W") < a.arg("rate") < a.arg("H") <= a.arg("rate") + 2]
        ok = ok and len(big) == 1
        dy = e.dy_buf is not None and _ptr(e.dy_buf)
        scales = [a.arg("in_scale") for a in gaps]
        if mode == "bn":    # sum(cA*g + cC), sum(cB*y), their sum
            return ok and len(gaps) == 2 and scales[0] is not None and scales[1] is not None and "dl3_affine_add" in b
        if mode == "dy":
            return ok and len(gaps) == 1 and scales[0] is None and gaps[0].arg("x") == dy
        if mode == "plain":
            return ok and len(gaps) == 1 and scales[0] is None and gaps[0].arg("x") != dy and not cat_consumer_has_bn(e)
        return ok
    return pred


def cat_consumer_has_bn(e):
    return bool(_buf(e, "concat_projection").bns)


def p_aspp_dropout(e):
    gf = ops(e.ops_bwd, "dl3_grad_finish")
    return (p_aspp_split("dy")(e) and any(a.arg("drop_rate") > 0 for a in gf)
            and any(a.arg("drop_seed") > 0 for a in ops(e.ops_fwd, "dl3_affine_add")))


def p_aspp_materialised(e):
    cat = _cat(e)
    rz = ops(e.ops_fwd, "dl3_resize_bilinear_fwd")
    b = names(e.ops_bwd)
    i = b.index("dl3_gap_fwd") if "dl3_gap_fwd" in b else -1
    return (id(cat) not in e.bcast_src and len(rz) == 1 and vals(rz[0], "Hi", "Wi") == [1, 1]
            and rz[0].arg("y") == cat.t.data_ptr() + 4 * 48
            and "dl3_resize_bilinear_bwd" not in b and i >= 0 and b[i + 1] == "dl3_grad_finish"
            and "dl3_pwconv_fwd_add" not in names(e.ops_fwd))


def p_decoder(swap, plain, twice=False):
    def pred(e):
        cat = _cat(e, "dec_cat")
        rz = ops(e.ops_fwd, "dl3_resize_bilinear_fwd")
        rb = ops(e.ops_bwd, "dl3_resize_bilinear_bwd")
        off = rz[0].arg("y") - _ptr(cat.t)
        src = _buf(e, "drop") if plain else _buf(e, "down_pointwise")
        ok = len(rz) == (2 if twice else 1) and off == (4 * 8 if swap else 0) and rz[0].arg("ldy") == cat.ld
        # the skip projection writes the other slice
        pw = [a for a in ops(e.ops_fwd, "dl3_pwconv_fwd") if a.arg("ldy") == cat.ld]
        ok = ok and len(pw) == 1 and pw[0].arg("y") - _ptr(cat.t) == (0 if swap else 4 * 24)
        if plain:     # straight into the source's gradient buffer
            ok = ok and all(vals(a, "dx", "lddx") == [_ptr(src.grad), src.ld] for a in rb)
            ok = ok and [a.arg("accumulate") for a in rb] == ([0, 1] if twice else [0])
        else:         # through tmp and dl3_grad_finish: the source carries BatchNorm and an activation
            b = names(e.ops_bwd)
            ok = (ok and len(rb) == 1 and rb[0].arg("dx") != _ptr(src.grad)
                  and b[b.index("dl3_resize_bilinear_bwd") + 1] == "dl3_grad_finish")
        return ok
    return pred


def p_head(form, folded=None, fused_loss=True):
    def pred(e):
        f, b = names(e.ops_fwd), names(e.ops_bwd)
        if form == "bilinear" and folded:
            return (e.head.form == "bilinear" and "dl3_upsample_softmax_xent_fold" in f and "dl3_resize_bilinear_bwd_rows" in b
                    and "dl3_resize_bilinear_fwd" not in f and e.loss_head.folded is not None)
        if form == "bilinear":
            return (e.head.form == "bilinear" and "dl3_upsample_softmax_xent" in f and "dl3_resize_bilinear_bwd" in b
                    and "dl3_resize_bilinear_bwd_rows" not in b and e.loss_head.folded is None)
        if form == "shuffle" and fused_loss:
            return (e.head.form == "shuffle" and e.loss_head.form == "shuffle" and "dl3_shuffle_softmax_xent" in f
                    and "dl3_phase_shift" not in f + b)
        if form == "shuffle":
            return (e.head.form == "shuffle" and e.loss_head.form == "plain" and "dl3_softmax_xent" in f
                    and f.count("dl3_phase_shift") == 1 and b.count("dl3_phase_shift") == 1)
        return e.head.form == "plain" and "dl3_softmax_xent" in f and "dl3_resize_bilinear_fwd" not in f
    return pred


def p_stems(e):
    f, b = names(e.ops_fwd), names(e.ops_bwd)
    d = ops(e.ops_fwd, "dl3_conv3x3_fwd")
    sink = ops(e.ops_bwd, "dl3_conv3x3_mfma_bwd_data")
    return (len(d) == 1 and vals(d[0], "Cin", "Cout", "stride") == [3, 32, 2] and "dl3_conv3x3_mfma_fwd" in f and "dl3_conv3x3_mfma_bwd_weight" in b
            and "dl3_conv3x3_bwd_weight" in b and "dl3_conv3x3_bwd_data" not in b
            # the MFMA bwd-data masks with the input's activation and reduces its BatchNorm's sums
            and len(sink) == 1 and sink[0].arg("in_act") == 1 and sink[0].arg("in_scale") is not None
            and sink[0].arg("x_mean") is not None)


def p_frozen_res(e):
    p = names(e.ops_prep)
    return (not e.bn_batch and p.count("dl3_bn_frozen_centered") == 3 and p.count("dl3_bn_frozen") == 1
            and "dl3_bn_finalize_direct" not in names(e.ops_fwd) and len(_buf(e, "stem").centred) == 1
            and all(a.arg("batch_mode") == 0 for a in ops(e.ops_bwd, "dl3_bn_bwd_finalize")) and p_residual(e))


def p_frozen_aspp(e):
    rows = ops(e.ops_fwd, "dl3_pwconv_fwd_rows")
    add = ops(e.ops_fwd, "dl3_pwconv_fwd_add")
    proj = _buf(e, "concat_projection")
    # the per-image unit of the split projection subtracts the moving mean; the per-pixel GEMM keeps a free bias slot
    return (not e.bn_batch and len(rows) == 2 and rows[1].arg("bias") == proj.vptr(7) and add[0].arg("bias") is None
            and 0 in proj.centred
            and sorted(_cat(e).centred) == [0, 16, 32])


def p_pruned(e):
    b = names(e.ops_bwd)
    frozen = [u for u in e.units if not u.outv.buf.requires_grad]
    mid = [a for a in ops(e.ops_bwd, "dl3_pwconv_bwd_weight") if a.arg("dbias") is not None and vals(a, "K", "N") == [16, 16]]
    return (len(frozen) == 5 and not any(e.trainable(n) for n in e.slots if n.startswith(("stem", "b1_")))
            and b.count("dl3_dwconv3x3_bwd") == 1 and len(mid) == 1
            and not any(vals(a, "K", "N", "in_act") == [16, 16, 0] for a in ops(e.ops_bwd, "dl3_pwconv_bwd_data")))


def p_pad_residual(e):
    return [b.ld for b in e.bufs if b.name in ("stem", "b1_expand", "b1_add")] == [6, 12, 6] and p_residual(e)


def p_pad_concat(e):
    return _cat(e).ld == 18 and [o for _, o, _ in _cat(e).bns] == [0, 6, 12] and p_aspp_split("bn")(e)


def p_728(e):
    return (_buf(e, "wide").ld == 736 and e.slots["wide/kernel:0"][3] == (1, 1, 8, 736)
            and e.slots["s1_depthwise/depthwise_kernel:0"][3] == (3, 3, 736, 1) and e.hshape["wide/kernel:0"] == (1, 1, 8, 728))


def p_epilogue_stats(e):
    f = names(e.ops_fwd)
    return f.count("dl3_bn_finalize") == 4 and "dl3_bn_finalize_direct" not in f and p_residual(e)


def p_relu_of_relu(e):
    d = ops(e.ops_fwd, "dl3_dwconv3x3_fwd")
    return len(d) == 1 and d[0].arg("in_act") == 1 and d[0].arg("in_scale") is not None


def p_two_bn_add(e):
    b = names(e.ops_bwd)
    u = _adds(e)[0]
    g = u.outv.buf.grad
    gf = ops(e.ops_bwd, "dl3_grad_finish")
    # both inputs alias g; each pass reads and writes g in place (no mask: the identity) and reduces its own buffer's sums
    return (len(gf) == 2 and u.a.buf.grad is g and u.b.buf.grad is g and all(a.arg("gin") == a.arg("gout") == _ptr(g) for a in gf)
            and {a.arg("xraw") for a in gf} =={_ptr(u.a.buf.t), _ptr(u.b.buf.t)})


def both(*preds):
    return lambda e: all(p(e) for p in preds)


# ---------------------------------------------------------------------------------------------------- the table
S = (20, 16, 8)      # H, W, input channels of most cases
S2 = (40, 32, 8)     # in front of a stride-2 layer
RES = ("res.addend_parked_then_taken", "res.add_gradient_aliased", "res.prestat_through_add")

CASES = [
    case("ir_noskip_s2", ir_noskip, 2, S2, ["ir.zeropad_valid_depthwise", "ir.dy_mat_single_tensor"], both(p_zeropad, p_dy_on)),
    case("ir_noskip_s2_dy_off", ir_noskip, 2, S2, ["ir.dy_mat_off_two_tensor"], both(p_zeropad, p_dy_off), env={"DL3_DY_MAT": "0"}),
    case("ir_res", ir_res(), 2, S, RES, p_residual),
    case("ir_res_stacked", ir_res(blocks=2), 2, S, RES + ("res.add_feeds_add",), p_stacked),
    case("ir_res_fused", ir_res(blocks=2), 2, S, ["fused.residual_addend", "fused.sums_against_other_tensor"], p_fused,
         env={"DL3_FUSED_ROWS": "1"}),
    case("ir_wide_fused", ir_wide, 2, S, ["fused.sup1_wide_k"], p_fused_sup1, env={"DL3_FUSED_ROWS": "1"}),
    case("ir_res_fork", ir_res(blocks=2), 2, S, ["fork.turns_dy_and_fused_off"], both(p_fork, p_stacked),
         env={"DL3_FUSED_ROWS": "1", "DL3_FORK": "1"}),
    case("xc_conv_shortcut", xc_conv_shortcut, 2, S2, ["xc.subsample_shortcut", "xc.sepconv_depth_activation_on",
                                                       "xc.sepconv_depth_activation_off"], p_subsample),
    case("xc_sum_skip", xc_sum_skip(), 2, S, ["xc.sum_skip_depthwise_sx"], p_dw_sx),
    case("xc_sum_skip_gather", xc_sum_skip(), 2, S, ["xc.sum_skip_gather_grad_finish"], p_dw_gather, kw={"dw_impl": 1}),
    case("aspp", aspp(), 4, S, ["aspp.gap", "aspp.rows_gemm_bn_direct", "aspp.rate_exceeds_map", "aspp.bn_at_concat_offsets",
                                "aspp.img_add_from_materialised_dy", "aspp.dropout_mask"], p_aspp_dropout, kw={"dropout": True}),
    case("aspp_dy_off", aspp(dropout=False), 4, S, ["aspp.img_add_bn_path"], p_aspp_split("bn"), env={"DL3_DY_MAT": "0"}),
    case("aspp_plain_projection", aspp(proj_bn=False, dropout=False), 4, S, ["aspp.img_add_plain_path"], p_aspp_split("plain")),
    case("aspp_pool_last", aspp(first=False, dropout=False), 4, S, ["aspp.resize_from_1x1_materialised"], p_aspp_materialised),
    case("decoder", decoder(), 2, S2, ["dec.resize_plain_backward", "dec.skip_projection_slice"], p_decoder(False, True),
         kw={"dropout": True}),
    case("decoder_swapped", decoder(swap=True), 2, S2, ["dec.resize_into_slice_offset"], p_decoder(True, True),
         kw={"dropout": True}),
    case("decoder_no_dropout", decoder(swap=True, dropout=False), 2, S2, ["dec.resize_backward_through_tmp"],
         p_decoder(True, False)),
    case("decoder_twice", decoder(twice=True), 2, S2, ["dec.resize_source_holds_gradient"], p_decoder(False, True, True),
         kw={"dropout": True}),
    case("head_bilinear_folded", head_only("bilinear"), 2, S2, ["head.bilinear_folded"], p_head("bilinear", True)),
    case("head_bilinear_unfolded", head_only("bilinear"), 2, S2, ["head.bilinear_unfolded"], p_head("bilinear", False),
         patch="no_fold"),
    case("head_shuffle", head_only("shuffle"), 2, S, ["head.shuffle_loss_head"], p_head("shuffle")),
    case("head_shuffle_unfused", head_only("shuffle"), 2, S, ["head.shuffle_not_head"], p_head("shuffle", fused_loss=False),
         env={"DL3_FUSE_SHUFFLE": "0"}),
    case("head_plain", head_only("plain"), 2, S, ["head.plain"], p_head("plain")),
    case("stems", stems, 2, (40, 32, 3), ["stem.direct_3_to_32_stride2", "stem.mfma_32_to_64_sink_into_bn_act"], p_stems),
    case("frozen_res", ir_res(), 2, S, ["frozen.centred_1x1", "frozen.gamma_beta_only"], p_frozen_res, kw={"bn_mode": "frozen"}),
    case("frozen_aspp", aspp(dropout=False), 4, S, ["frozen.split_concat_img_unit_offset"], p_frozen_aspp,
         kw={"bn_mode": "frozen"}),
    case("pruned", pruned, 2, S, ["prune.below_cut", "prune.bias_arm_on_pruned_input"], p_pruned),
    # (6 and 12: the block's tensors and its Add are 6 wide; the depthwise kernels take multiples of 4 only — 6 / 10 is
    # refuse_depthwise_width below)
    case("pad_residual", ir_res(widths=(6, 12)), 2, S, ["pad.residual_odd_widths"], p_pad_residual),
    case("pad_concat", aspp(dropout=False, widths=(12, 6, 10)), 4, S, ["pad.concat_odd_widths"], p_pad_concat),
    case("pad_728", wide_728, 2, (16, 16, 8), ["pad.728_stored_736"], p_728),
    case("odd_res_b3", ir_res(), 3, S, ["odd.residual_b3"], p_residual),
    case("odd_aspp_b3", aspp(dropout=False), 3, S, ["odd.aspp_b3"], p_aspp_split("dy"), seeds=(2, 3, 4, 5, 6, 7)),
    case("res_epilogue_stats", ir_res(), 2, (48, 48, 8), ["extra.bn_epilogue_stats_above_4096_rows"], p_epilogue_stats),
    case("relu_of_relu", relu_of_relu, 2, S, ["extra.relu_of_relu_view"], p_relu_of_relu),
    case("add_of_two_bn", add_of_two_bn, 2, S, ["extra.grad_finish_alias_without_prestat"], p_two_bn_add),
    case("refuse_elementwise_slice", refuse_elementwise_slice, 2, S, ["refuse.elementwise_into_slice"], None,
         raises="element-wise gradient into a channel slice"),
    case("refuse_stats_slice", refuse_slice_consumer(True), 2, S, ["refuse.bn_stats_through_slice"], None,
         raises="BN-backward statistics through a channel slice"),
    case("refuse_partial_first", refuse_slice_consumer(False), 2, S, ["refuse.partial_first_contribution"], None,
         raises="first gradient contribution into a channel slice"),
    case("refuse_depthwise_width", ir_res(widths=(6, 10)), 2, S, ["refuse.depthwise_width_not_multiple_of_4"], None,
         raises="depthwise conv over 10 channels"),
    case("refuse_foreign_addend", refuse_foreign_addend, 2, S, ["refuse.resize_foreign_addend"], None,
         kw={"dropout": True}, raises="resize backward with a foreign addend"),
]
BY_NAME = {c.name: c for c in CASES}
RUNNABLE = [c for c in CASES if c.raises is None]


# ---------------------------------------------------------------------------------------------------- inputs
def build(c, seed=None):
    """the case's model with seeded weights: glorot kernels (graph.clear_session's stream), random biases, randomised
    BatchNorm parameters and moving statistics"""
    import dl3_amd  # noqa: F401
    from dl3_amd import graph as G
    seed = c.seeds[0] if seed is None else seed
    G.clear_session(seed=seed)
    model = c.build(G, c.shape)
    rng = np.random.default_rng(1000 + seed)
    for l in model.layers:
        if not l.weights:
            continue
        ws = []
        for n, w in l.weights.items():
            if n.endswith("/gamma:0"):
                w = rng.uniform(0.5, 1.5, w.shape)
            elif n.endswith("/beta:0"):
                w = rng.normal(0.0, 0.3, w.shape)
            elif n.endswith("/moving_mean:0"):
                w = rng.normal(0.0, 0.2, w.shape)
            elif n.endswith("/moving_variance:0"):
                w = rng.uniform(0.5, 1.5, w.shape)
            elif n.endswith("/bias:0"):
                w = rng.normal(0.0, 0.2, w.shape)
            elif n.endswith("/depthwise_kernel:0"):
                w = rng.normal(0.0, 0.35, w.shape)     # (glorot over 9*C fan-in would leave a depthwise output near zero)
            ws.append(np.asarray(w, np.float32))
        l.set_weights(ws)
    return model


def batch(c, model, seed=None):
    """(x, labels, sample weights) of the case: normal inputs (raw pixels where the graph prescales), labels with void
    pixels, weights in [0.5, 2) and zero on void"""
    seed = c.seeds[0] if seed is None else seed
    rng = np.random.default_rng(2000 + seed)
    if any(l.kind == "Prescale" for l in model.layers):
        x = rng.integers(0, 256, (c.B,) + tuple(c.shape)).astype(np.float32)
    else:
        x = rng.normal(0, 1, (c.B,) + tuple(c.shape)).astype(np.float32)
    hw = model.output.shape[0]
    labels = rng.integers(0, CLASSES + 1, (c.B, hw)).astype(np.float32)
    sw = ((labels < CLASSES) * rng.uniform(0.5, 2.0, labels.shape)).astype(np.float32)
    return x, labels, sw


def dropout_layers(c, model):
    """[(Dropout layer, output shape with the batch axis)] of an engine built with dropout on"""
    if not c.kw.get("dropout"):
        return []
    return [(l, (c.B,) + tuple(l.output.shape)) for l in model._topo if l.kind == "Dropout" and l.cfg["rate"] > 0]


def engine_seed(c):
    """Engine(seed=...) of the case: distinct per case, so that graph.Model._engine never hands back another test's engine"""
    return 7000 + [k.name for k in CASES].index(c.name)


def engine_kw(c, use_graph=False):
    kw = dict(dropout=False, use_graph=use_graph, seed=engine_seed(c))
    kw.update(c.kw)
    return kw


def masks(c, model):
    """{Dropout layer name: keep mask [B,H,W,C]} of the engine's first step (rank 0: Engine.seed is the keyword)"""
    from tests.gpu_util import dropout_keep_mask
    return {l.name: dropout_keep_mask(engine_seed(c), int(np.prod(shp)), l.cfg["rate"]).reshape(shp).astype(np.float64)
            for l, shp in dropout_layers(c, model)}


def reference(c, model, data, dtype):
    from tests import graph_ref
    x, labels, sw = data
    return graph_ref.run(model, x, labels, sw, dtype=dtype, bn_mode=c.kw.get("bn_mode", "batch"),
                         dropout_masks=masks(c, model))


_SEEDS = {}


def seed_of(c, margin=0.02):
    """the first of the case's fixed seeds whose float64 pre-activations on FEW-ROW tensors (<= 64 rows per channel: the
    image-pooling branch, whose BatchNorm sees one row per image) stay `margin` clear of the activation's kinks — there
    a float32 run may rectify an element the float64 run lets through, which is conditioning, not wiring"""
    import torch
    from tests import graph_ref
    if c.name in _SEEDS:
        return _SEEDS[c.name]
    for seed in c.seeds:
        model = build(c, seed)
        few = [l for l in model._topo if l.kind == "Activation" and l.cfg["fn"] != "softmax"
               and c.B * int(np.prod(l.output.shape[:-1])) <= 64]
        if not few:
            break
        x, labels, sw = batch(c, model, seed)
        r = graph_ref.run(model, x, labels, sw, dtype=torch.float64, bn_mode=c.kw.get("bn_mode", "batch"),
                          dropout_masks=masks(c, model), keep=[l.inbound[0].layer.name for l in few])
        gaps = [np.abs(v - k).min() for l in few for v in [r.values[l.inbound[0].layer.name]]
                for k in ((0.0, 6.0) if l.cfg["fn"] == "relu6" else (0.0,))]
        if min(gaps) > margin:
            break
    else:
        raise AssertionError("%s: no seed of %s keeps the few-row pre-activations clear of zero" % (c.name, c.seeds))
    _SEEDS[c.name] = seed
    return seed


_PREPARED = {}


def prepared(c):
    """(model, (x, labels, sw), float64 reference, float32 reference) of the case at its chosen seed: computed once per
    process and shared by every test that needs it (the model's host weights are never changed afterwards: engines
    read them, a test that trains writes back through its own engine only)"""
    import torch
    if c.name not in _PREPARED:
        seed = seed_of(c)
        model = build(c, seed)
        data = batch(c, model, seed)
        _PREPARED[c.name] = (model, data, reference(c, model, data, torch.float64), reference(c, model, data, torch.float32))
    return _PREPARED[c.name]
