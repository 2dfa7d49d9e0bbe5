"""The output head as a kernel that reads class scores sees it.

Three forms: `plain` — materialised logits; `bilinear` — the low-resolution logits in front of the final
dl3_resize_bilinear_fwd; `shuffle` — the unshuffled Subpixel output in front of dl3_phase_shift.  Five kernel families take
any of them (the focal loss, §18, in the forms of the cross-entropy it stands in for); the two of the soft-Jaccard loss
(§16) take `plain` and `bilinear`.  Engine._lo_softmax decides the form
once; each consumer admits it by a rule of its own or reads the same head as `plain`; KERNELS is the one place that names the entry points and their argument order."""

_LOSS = ("src", "labels", "w", "nnz", "grad", "part", "dims")
_FOCAL = ("src", "labels", "w", "nnz", "alpha", "gamma", "grad", "part")
_EVAL = ("src", "labels", "w", "part", "loss", "nnz", "counts", "confusion", "mask")
# family -> form -> (entry point, arguments).  A string is a value the caller names, or one of the head's dimension tuples
# ("rows": M, C; "images": B, HW, C; "dims": the form's own); anything else is passed as it stands.
KERNELS = {
    "loss": {"plain": ("dl3_softmax_xent", ("src", "labels", "w", "nnz", None, "grad", "part", "rows")),
             "bilinear": ("dl3_upsample_softmax_xent", ("src", "labels", "w", "nnz", None, "grad", "part", "dims")),
             # grad: each output row folded onto the low-resolution columns (the resize unit's backward folds the rows)
             "bilinear_fold": ("dl3_upsample_softmax_xent_fold", _LOSS),
             "shuffle": ("dl3_shuffle_softmax_xent", _LOSS)},
    # the focal loss: the `loss` family's forms, grids and partials, alpha (device pointer or None) and gamma on top
    "focal_loss": {"plain": ("dl3_focal_xent", _FOCAL + ("rows",)),
                   "bilinear": ("dl3_upsample_focal_xent", _FOCAL + ("dims",)),
                   "bilinear_fold": ("dl3_upsample_focal_xent_fold", _FOCAL + ("dims",)),
                   "shuffle": ("dl3_shuffle_focal_xent", _FOCAL + ("dims",))},
    "pixel_xent": {"plain": ("dl3_pixel_xent_plain", ("src", "labels", "w", "out", "rows")),
                   "bilinear": ("dl3_pixel_xent_bilinear", ("src", "labels", "w", "out", "dims")),
                   "shuffle": ("dl3_pixel_xent_shuffle", ("src", "labels", "w", "out", "dims"))},
    # the soft-Jaccard loss: per-image sums, then loss + full-resolution gradient (no folded, no shuffle form)
    "jaccard_sums": {"plain": ("dl3_jaccard_sums_plain", ("src", "labels", "w", "out", "images")),
                     "bilinear": ("dl3_jaccard_sums_bilinear", ("src", "labels", "w", "out", "dims"))},
    "jaccard_loss": {"plain": ("dl3_softmax_xent_jaccard", ("src", "labels", "w", "nnz", "coef", "lam", "grad", "part",
                                                            "images")),
                     "bilinear": ("dl3_upsample_softmax_xent_jaccard", ("src", "labels", "w", "nnz", "coef", "lam", "grad",
                                                                        "part", "dims"))},
    "eval_tail": {"plain": ("dl3_eval_tail_plain", _EVAL + ("images",)),
                  "bilinear": ("dl3_eval_tail_bilinear", _EVAL + ("dims",)),
                  "shuffle": ("dl3_eval_tail_shuffle", _EVAL + ("dims",))},
    "crf_unary": {"plain": ("dl3_crf_unary_plain", ("src", 0, "U", "images", "scale", "clip")),
                  "bilinear": ("dl3_crf_unary_bilinear", ("src", "U", "dims", "scale", "clip")),
                  "shuffle": ("dl3_crf_unary_shuffle", ("src", "U", "dims", "scale", "clip"))},
}


class Head:
    """form; unit: the ResizeUnit / ShuffleUnit behind a fused form; op: the ONE launch record that materialises the
    full-resolution logits `v` from `src`, the view the fused kernels read (plain: src is v, no unit, no op); plain: the
    same head read as `plain`; folded: the column-folded gradient the training loss left for unit.bwd (else None)"""

    def __init__(self, B, v, form="plain", unit=None, op=None):
        self.form, self.v, self.unit, self.op, self.folded = form, v, unit, op, None
        self.src = v if unit is None else unit.inv
        self.sizes = {"rows": (v.buf.M, v.C), "images": (B, v.buf.M // B, v.C)}
        if form == "bilinear":
            self.sizes["dims"] = (B,) + tuple(unit.dims[1:5]) + (v.C,)              # B, Hi, Wi, Ho, Wo, C
        elif form == "shuffle":
            self.sizes["dims"] = (B, unit.inv.buf.H, unit.inv.buf.W, v.C, unit.r)    # B, H, W, C, r
        self.plain = self if form == "plain" else Head(B, v)

    def entry(self, family, fold=False):
        return KERNELS[family][self.form + ("_fold" if fold else "")]

    def dims(self, family):
        return next(self.sizes[s] for s in self.entry(family)[1] if s in self.sizes)

    def launch(self, family, fold=False, **vals):
        """(entry point, *arguments) of `family` on this head — what Engine.op takes behind its list"""
        name, slots = self.entry(family, fold)
        vals["src"] = self.src.p()
        args = [name]
        for s in slots:
            if s in self.sizes:
                args += self.sizes[s]
            else:
                args.append(vals[s] if isinstance(s, str) else s)
        return args
