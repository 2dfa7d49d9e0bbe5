"""Dense-CRF post-processing on the device: the exact mean-field inference of the model the reference's do_crf
configures in pydensecrf (utils.py:74-91) — unary energies from the labels, a Gaussian position kernel, a bilateral
position + colour kernel, symmetric normalisation, Potts compatibility, parallel updates — summed over ALL pixel pairs by
dl3_crf_inference (csrc/crf.hip) instead of pydensecrf's permutohedral lattice [pydensecrf-semantics].
Results agree with pydensecrf only as far as its lattice approximates these sums.

The unary energies are built on the host in numpy (O(N L)); every parameter comes from utils.CRF_PARAMS.
"""
import numpy as np

from . import capi

MAX_LABELS = 32
PAD_ENERGY = 1e30  # unary of the labels an image of a batch does not have: exp(-1e30 - max) == 0 exactly


def unary_from_labels(labels, n_labels, gt_prob, zero_unsure=True):
    """pydensecrf.utils.unary_from_labels [pydensecrf-semantics]: float32 [n_labels, N].  The given label of a pixel costs
    -log(gt_prob), every other one -log((1 - gt_prob) / (n_labels - 1)).  With zero_unsure label 0 means "no label"
    (all energies -log(1 / n_labels)) and label k >= 1 owns row k - 1; row n_labels - 1 is then written only through the
    negative index of label 0 and overwritten by the unsure value."""
    labels = np.asarray(labels).reshape(-1)
    n_energy = -np.log((1.0 - gt_prob) / (n_labels - 1))
    p_energy = -np.log(gt_prob)
    U = np.full((n_labels, labels.size), n_energy, dtype="float32")
    U[labels - 1 if zero_unsure else labels, np.arange(U.shape[1])] = p_energy
    if zero_unsure:
        U[:, labels == 0] = -np.log(1.0 / n_labels)
    return U


def kernel_params():
    """{sx, sy, w_gauss, sxy, srgb, w_bilateral} of dl3_crf_inference from utils.CRF_PARAMS"""
    from .utils import CRF_PARAMS as P
    sx, sy = P["gaussian_sxy"]
    return np.array([sx, sy, P["gaussian_compat"], P["bilateral_sxy"], P["bilateral_srgb"], P["bilateral_compat"]],
                    np.float32)


def inference(images, U, iters, want_q=False, want_energy=False):
    """dl3_crf_inference on the current stream: images uint8 cuda [B,H,W,3], U float32 cuda [B,L,N] ->
    (map int32 [B,N], Q or None, energy or None), device tensors"""
    import torch
    B, H, W = images.shape[:3]
    L = U.shape[1]
    dev = images.device
    ws = torch.empty(int(capi.lib().dl3_crf_workspace_bytes(B, H, W, L)) or 16, dtype=torch.uint8, device=dev)
    par = torch.from_numpy(kernel_params())  # read by the host side of the launch
    MAP = torch.empty(B, H * W, dtype=torch.int32, device=dev)
    Q = torch.empty(B, L, H * W, dtype=torch.float32, device=dev) if want_q else None
    E = torch.empty(B, L, H * W, dtype=torch.float32, device=dev) if want_energy else None
    capi.call("dl3_crf_inference", images.data_ptr(), U.data_ptr(), B, H, W, L, par.data_ptr(), int(iters),
              Q.data_ptr() if want_q else None, E.data_ptr() if want_energy else None, MAP.data_ptr(), ws.data_ptr(),
              ws.numel(), torch.cuda.current_stream().cuda_stream)
    return MAP, Q, E


def dense_crf(images, masks, zero_unsure=True, return_q=False):
    """do_crf for a batch of images of one size.  images [B,H,W,3] (cast to uint8 as the reference does), masks [B,H,W]
    integer; numpy arrays or cuda tensors.  Per image: colors, labels = np.unique(mask) as in do_crf, the unary energies
    padded to the batch's largest label count with a large finite energy (those labels keep probability exactly 0, so an
    image's result does not depend on its batch), one dl3_crf_inference launch sequence for the batch, and the
    reference's label restore (utils.restore_crf_labels, quirk included).

    Returns int64 masks [B,H,W] — a cuda tensor when `masks` is one (the pixels never visit the host; only the small
    integer masks do, for np.unique and the unary), else a numpy array — and with return_q also Q [B,L,H*W] (rows of the
    padding labels are 0).  An image whose mask has a single value comes back unchanged (the unary divides by
    n_labels - 1; pydensecrf does not define that case)."""
    import torch
    from .utils import CRF_PARAMS, restore_crf_labels
    if not torch.cuda.is_available():
        raise capi.DL3Error("the device dense-CRF needs a GPU (HIP device); there is no CPU fallback")
    on_device = torch.is_tensor(masks)
    mh = masks.detach().cpu().numpy() if on_device else np.asarray(masks)
    if mh.ndim != 3:
        raise ValueError("masks must be [B,H,W], got shape %r" % (mh.shape,))
    B, H, W = mh.shape
    if tuple(images.shape) != (B, H, W, 3):
        raise ValueError("images must be [B,H,W,3] matching the masks, got %r for masks %r" % (tuple(images.shape), mh.shape))
    dev = masks.device if on_device else torch.device("cuda", torch.cuda.current_device())
    if torch.is_tensor(images):
        im = images.to(dev).to(torch.uint8).contiguous()
    else:
        im = torch.from_numpy(np.ascontiguousarray(np.asarray(images).astype("uint8"))).to(dev)
    uniq = [np.unique(mh[b], return_inverse=True) for b in range(B)]
    L = max(len(c) for c, _ in uniq)
    if L > MAX_LABELS:
        raise capi.DL3Error("dense_crf: a mask with %d distinct values; the device kernels take at most %d labels"
                            % (L, MAX_LABELS))
    out = torch.from_numpy(mh.astype(np.int64)).to(dev) if not on_device else masks.to(torch.int64).clone()
    Qout = torch.zeros(B, L, H * W, dtype=torch.float32, device=dev) if return_q else None
    live = [b for b in range(B) if len(uniq[b][0]) > 1]
    if live:
        U = np.full((len(live), L, H * W), PAD_ENERGY, np.float32)
        for n, b in enumerate(live):
            colors, labels = uniq[b]
            U[n, :len(colors)] = unary_from_labels(labels.reshape(-1), len(colors), CRF_PARAMS["gt_prob"], zero_unsure)
        idx = torch.tensor(live, device=dev)
        MAP, Q, _ = inference(im[idx] if len(live) < B else im, torch.from_numpy(U).to(dev), CRF_PARAMS["iterations"],
                              want_q=return_q)
        MAP = MAP.to(torch.int64)
        for n, b in enumerate(live):
            # restore_crf_labels acts on values: run the reference's loop on the indices present and apply it as a table
            present = torch.unique(MAP[n]).cpu().numpy()
            table = np.arange(L, dtype=np.int64)
            table[present] = restore_crf_labels(present.copy(), uniq[b][0])
            out[b] = torch.from_numpy(table).to(dev)[MAP[n]].reshape(H, W)
            if return_q:
                Qout[b] = Q[n]
    if not on_device:
        out = out.cpu().numpy()
        Qout = Qout.cpu().numpy() if return_q else None
    return (out, Qout) if return_q else out
