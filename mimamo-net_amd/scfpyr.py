"""SCFpyr_PyTorch on MI355X -- drop-in for api/steerable/SCFpyr_PyTorch.py:51-318.

`build(im_batch)` returns the reference's full list `[hi, [band_0..band_{nbands-1}], ..., lo]` for arbitrary
square images, and `reconstruct(coeff)` turns such a list -- edited or not -- back into the image batch `[N,H,W]`;
the arithmetic runs in libmimamo_hip.so (csrc/scfpyr.hip: DFT-by-summation with float64 accumulation).  The
inference pipeline does not use this class -- Phase_Difference_Extractor.build_pyramid calls the mirrored-input
kernel of csrc/pyramid.hip, which produces only the coefficients the phase stage keeps.

Both methods are differentiable, like the reference's torch-op pyramid: when grad mode is on and an input requires grad
they run through the autograd Functions at the end of this file, whose backward passes are the native adjoints
(mm_scfpyr_build_adjoint / mm_scfpyr_reconstruct_adjoint).  Both operators are linear, so each backward is the opposite
direction's operator, and it is itself differentiable (double backward works).
"""
import ctypes

import numpy as np
import torch

from . import _lib


class SCFpyr_PyTorch(object):
    def __init__(self, height=5, nbands=4, scale_factor=2, device=None, precision=32):
        """Arguments as SCFpyr_PyTorch.py:51-58.  Unlike the reference this does NOT call
        torch.set_default_dtype (quirk Q10) and the device must be a ROCm device."""
        self.height = height
        self.nbands = nbands
        self.scale_factor = scale_factor
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError("SCFpyr_PyTorch: this build has no CPU path; pass a ROCm device")
        self.precision = precision
        assert self.precision in [32, 64]
        self.dtype = torch.float32 if precision == 32 else torch.float64
        self._handle = None
        self._size = None

    def _get(self, size):
        if self._handle is None or self._size != size:
            self.close()
            h = ctypes.c_void_p()
            with torch.cuda.device(self.device):
                rc = _lib.lib().mm_scfpyr_create(ctypes.byref(h), int(size), int(self.height), int(self.nbands),
                                                 int(self.scale_factor))
            if rc == _lib.MM_ERR_TOO_SMALL:  # the reference formats the level count into the message (:91)
                raise RuntimeError('Cannot build {} levels, image too small.'.format(self.height))
            _lib.check(rc, "mm_scfpyr_create")
            self._handle, self._size = h, size
        return self._handle

    def close(self):
        if getattr(self, "_handle", None) is not None:
            _lib.lib().mm_scfpyr_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _output_shapes(self, h, n):
        L = _lib.lib()
        side, cplx = ctypes.c_int(), ctypes.c_int()
        shapes = []
        for i in range(L.mm_scfpyr_num_outputs(h)):
            _lib.check(L.mm_scfpyr_output_info(h, i, ctypes.byref(side), ctypes.byref(cplx)), "mm_scfpyr_output_info")
            shapes.append((n, side.value, side.value, 2) if cplx.value else (n, side.value, side.value))
        return shapes

    def _image_to_coeffs(self, x, size, adjoint=False):
        """x [N,1,size,size] or [N,size,size] -> the flat coefficient list: the build, or (adjoint) the vector-Jacobian
        product of reconstruct, which maps an image gradient to coefficient gradients of the build's shapes."""
        h = self._get(size)
        n = x.shape[0]
        L = _lib.lib()
        outs = [torch.empty(shape, dtype=self.dtype, device=self.device) for shape in self._output_shapes(h, n)]
        n_out = len(outs)
        ws_bytes = L.mm_scfpyr_workspace_bytes(h, n)
        ws = torch.empty((max(ws_bytes, 8) // 8,), dtype=torch.float64, device=self.device)
        ptrs = (ctypes.c_void_p * n_out)(*[o.data_ptr() for o in outs])
        x = x.contiguous()
        name = "mm_scfpyr_reconstruct_adjoint" if adjoint else "mm_scfpyr_build"
        with torch.cuda.device(self.device):
            rc = getattr(L, name)(h, _lib.ptr(x), self.precision, n, ptrs, _lib.ptr(ws), ws_bytes, _lib.current_stream())
        _lib.check(rc, name)
        return outs

    def _coeffs_to_image(self, flat, size, adjoint=False):
        """flat coefficient list -> the image batch [N,size,size]: the reconstruct, or (adjoint) the vector-Jacobian product
        of build, which maps coefficient gradients to the image gradient."""
        h = self._get(size)
        n = flat[0].shape[0]
        out = torch.empty((n, size, size), dtype=self.dtype, device=self.device)
        L = _lib.lib()
        ws_bytes = L.mm_scfpyr_workspace_bytes(h, n)
        ws = torch.empty((max(ws_bytes, 8) // 8,), dtype=torch.float64, device=self.device)
        flat = [c.contiguous() for c in flat]
        ptrs = (ctypes.c_void_p * len(flat))(*[c.data_ptr() for c in flat])
        name = "mm_scfpyr_build_adjoint" if adjoint else "mm_scfpyr_reconstruct"
        with torch.cuda.device(self.device):
            rc = getattr(L, name)(h, ptrs, self.precision, n, _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.current_stream())
        _lib.check(rc, name)
        return out

    def build(self, im_batch):
        """im_batch [N,1,H,W] -> [hi [N,H,W], [bands [N,h,w,2]] per level ..., lo [N,h',w']]  (SCFpyr_PyTorch.py:70-125)."""
        assert im_batch.device == self.device, 'Devices invalid (pyr = {}, batch = {})'.format(self.device, im_batch.device)
        assert im_batch.dtype == self.dtype, 'Image batch must be torch.float{}'.format(self.precision)
        assert im_batch.dim() == 4, 'Image batch must be of shape [N,C,H,W]'
        assert im_batch.shape[1] == 1, 'Second dimension must be 1 encoding grayscale image'
        n, _, hh, ww = im_batch.shape
        if hh != ww:
            raise NotImplementedError("square images only (SCFpyr_PyTorch.py:87 swaps height and width)")
        if torch.is_grad_enabled() and im_batch.requires_grad:
            outs = list(_ImageToCoeffs.apply(self, hh, False, im_batch))
        else:
            outs = self._image_to_coeffs(im_batch, hh)
        coeff = [outs[0]]
        k = 1
        for _ in range(self.height - 2):
            coeff.append(outs[k:k + self.nbands])
            k += self.nbands
        coeff.append(outs[k])
        return coeff

    def reconstruct(self, coeff):
        """coeff = a list as build returns it, possibly edited -> the real image batch [N,H,W] in the pyramid's dtype on its
        device (SCFpyr_PyTorch.py:214-318).  Deliberate difference: with height 2 the list is [hi, lo] and the reference
        compares nbands with len(lo), the batch size (:216); here any batch size is accepted."""
        if not isinstance(coeff, (list, tuple)) or len(coeff) != self.height:
            raise ValueError("reconstruct: expected a list of {} levels (hi, {} band levels, lo)".format(
                self.height, self.height - 2))
        for level in coeff[1:-1]:
            if not isinstance(level, (list, tuple)) or len(level) != self.nbands:
                raise Exception("Unmatched number of orientations")
        flat = [coeff[0]] + [b for level in coeff[1:-1] for b in level] + [coeff[-1]]
        for c in flat:
            if not isinstance(c, torch.Tensor):
                raise ValueError("reconstruct: coefficients must be tensors")
            assert c.device == self.device, 'Devices invalid (pyr = {}, batch = {})'.format(self.device, c.device)
            assert c.dtype == self.dtype, 'Image batch must be torch.float{}'.format(self.precision)
        hi = flat[0]
        if hi.dim() != 3 or hi.shape[1] != hi.shape[2]:
            raise ValueError("reconstruct: the hi-pass residual must be [N,H,H], got {}".format(tuple(hi.shape)))
        n, size = hi.shape[0], hi.shape[1]
        h = self._get(size)
        shapes = self._output_shapes(h, n)
        for i, (c, shape) in enumerate(zip(flat, shapes)):
            if tuple(c.shape) != shape:
                raise ValueError("reconstruct: coefficient {} has shape {}, expected {}".format(i, tuple(c.shape), shape))
        if torch.is_grad_enabled() and any(c.requires_grad for c in flat):
            return _CoeffsToImage.apply(self, size, False, *flat)
        return self._coeffs_to_image(flat, size)


# The two directions as autograd Functions.  Both operators are linear, so no tensor is saved: the backward of an
# image -> coefficients map (the build, or the reconstruct adjoint) is the coefficients -> image map with the opposite
# `adjoint` flag, and vice versa, applied through the other Function so that the backward is itself differentiable.
# The backward resolves the native handle by size (pyr._get): between forward and backward the same pyramid object may
# have been used at another size, which replaces its handle.

class _ImageToCoeffs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pyr, size, adjoint, x):
        ctx.pyr, ctx.size, ctx.adjoint, ctx.x_shape = pyr, size, adjoint, x.shape
        return tuple(pyr._image_to_coeffs(x, size, adjoint))

    @staticmethod
    def backward(ctx, *grads):
        if not ctx.needs_input_grad[3]:
            return None, None, None, None
        g = _CoeffsToImage.apply(ctx.pyr, ctx.size, not ctx.adjoint, *[t.contiguous() for t in grads])
        return None, None, None, g.reshape(ctx.x_shape)


class _CoeffsToImage(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pyr, size, adjoint, *flat):
        ctx.pyr, ctx.size, ctx.adjoint = pyr, size, adjoint
        return pyr._coeffs_to_image(flat, size, adjoint)

    @staticmethod
    def backward(ctx, grad):
        need = ctx.needs_input_grad[3:]
        if not any(need):
            return (None,) * (3 + len(need))
        gs = _ImageToCoeffs.apply(ctx.pyr, ctx.size, not ctx.adjoint, grad.contiguous())
        return (None, None, None) + tuple(g if k else None for g, k in zip(gs, need))
