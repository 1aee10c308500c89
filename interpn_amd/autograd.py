"""A multilinear or multicubic `Interpolator` as a differentiable function of the observation coordinates.

`interp(it, obs)` evaluates `it` at the points given as torch CUDA tensors and takes part in torch's autograd: the
backward pass multiplies the incoming gradient by the derivative of the interpolant with respect to each coordinate,
which the forward pass computed in the same kernel (`Interpolator.eval_grad_tensors`, or `eval_cubic_grad_tensors` for a
handle whose `method` is "cubic").  The table is a constant of the
graph: the gradient with respect to `vals` is not built.

`interp_points(it, pts)` is the same for positions kept as ONE tensor of shape `(..., N)`: its forward pass is one
`Interpolator.eval_points_grad_tensors`, and `pts.grad` has the shape of `pts`.

`interp_fields(fs, obs)` is `interp` for a field set (`Fields`): a `(K, *shape)` tensor whose forward pass is one
`Fields.eval_grad_tensors`; the saved Jacobian turns the incoming `(K, *shape)` gradient into one gradient per coordinate.

`interp_fields_points(fs, pts)` is `interp_fields` for positions kept as ONE tensor of shape `(..., N)`: a `(..., K)` tensor
whose forward pass is one `Fields.eval_points_grad_tensors`; `pts.grad` has the shape of `pts`.

`interp_lattice(it, axes)` is `interp` on the lattice axes[0] x .. x axes[N-1]: its forward pass is one
`Interpolator.eval_lattice_grad_tensors`; the backward pass sums the incoming `(*m)` gradient times component d over every
lattice dimension but d, which gives one gradient per coordinate VECTOR.

`interp_fields_lattice(fs, axes, field_axis=0)` is `interp_lattice` for a field set: a `(K, *m)` or `(*m, K)` tensor whose
forward pass is one `Fields.eval_lattice_grad_tensors`; the backward pass sums the incoming gradient times `jac[f, d]` over
the fields and over every lattice dimension but d.

torch is imported on first use, and this module is not imported by `import interpn_amd`.
"""

from __future__ import annotations

_FUNCTION = None
_POINTS_FUNCTION = None
_FIELDS_FUNCTION = None
_FIELDS_POINTS_FUNCTION = None
_LATTICE_FUNCTION = None
_FIELDS_LATTICE_FUNCTION = None


def _function():
    """The torch.autograd.Function, built on first use so that importing this module does not import torch."""
    global _FUNCTION
    if _FUNCTION is not None:
        return _FUNCTION
    import torch

    class _Interp(torch.autograd.Function):
        @staticmethod
        def forward(ctx, it, *obs):
            shape = obs[0].shape
            flat = [o.detach().reshape(-1).contiguous() for o in obs]
            cubic = getattr(it, "method", None) == "cubic"
            out, grad = (it.eval_cubic_grad_tensors if cubic else it.eval_grad_tensors)(flat)
            it.finish()
            ctx.save_for_backward(grad)
            ctx.obs_shape = shape
            return out.reshape(shape)

        @staticmethod
        def backward(ctx, grad_out):
            (grad,) = ctx.saved_tensors
            g = grad_out.reshape(-1)
            res = [None]
            for d in range(grad.shape[0]):
                res.append((g * grad[d]).reshape(ctx.obs_shape) if ctx.needs_input_grad[d + 1] else None)
            return tuple(res)

    _FUNCTION = _Interp
    return _FUNCTION


def interp(it, obs):
    """Value of the multilinear or multicubic interpolator `it` at `obs` (a sequence of N equally shaped torch CUDA tensors of the
    handle's dtype), differentiable with respect to every tensor of `obs`."""
    return _function().apply(it, *obs)


def _points_function():
    """The point-major torch.autograd.Function, built on first use like `_function`."""
    global _POINTS_FUNCTION
    if _POINTS_FUNCTION is not None:
        return _POINTS_FUNCTION
    import torch

    class _InterpPoints(torch.autograd.Function):
        @staticmethod
        def forward(ctx, it, pts):
            shape = pts.shape
            flat = pts.detach().reshape(-1, shape[-1])
            if flat.shape[1] > 1 and flat.stride(1) != 1:
                flat = flat.contiguous()
            out, grad = it.eval_points_grad_tensors(flat)
            it.finish()
            ctx.save_for_backward(grad)
            ctx.pts_shape = shape
            return out.reshape(shape[:-1])

        @staticmethod
        def backward(ctx, grad_out):
            (grad,) = ctx.saved_tensors
            return None, (grad_out.reshape(-1).unsqueeze(-1) * grad).reshape(ctx.pts_shape)

    _POINTS_FUNCTION = _InterpPoints
    return _POINTS_FUNCTION


def interp_points(it, pts):
    """Value of the multilinear or multicubic interpolator `it` at the points `pts`, ONE torch CUDA tensor of shape `(..., N)`
    of the handle's dtype: the result has shape `pts.shape[:-1]` and is differentiable with respect to `pts`."""
    return _points_function().apply(it, pts)


def _fields_function():
    """The field-set torch.autograd.Function, built on first use like `_function`."""
    global _FIELDS_FUNCTION
    if _FIELDS_FUNCTION is not None:
        return _FIELDS_FUNCTION
    import torch

    class _InterpFields(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fs, *obs):
            shape = obs[0].shape
            flat = [o.detach().reshape(-1).contiguous() for o in obs]
            out, jac = fs.eval_grad_tensors(flat)
            fs.finish()
            ctx.save_for_backward(jac)
            ctx.obs_shape = shape
            return out.reshape((out.shape[0],) + tuple(shape))

        @staticmethod
        def backward(ctx, grad_out):
            (jac,) = ctx.saved_tensors  # (K, N, n)
            g = grad_out.reshape(jac.shape[0], -1)
            full = (g[:, None, :] * jac).sum(0)  # grad_obs[d] = sum_f grad_out[f] * J[f, d]
            res = [None]
            for d in range(jac.shape[1]):
                res.append(full[d].reshape(ctx.obs_shape) if ctx.needs_input_grad[d + 1] else None)
            return tuple(res)

    _FIELDS_FUNCTION = _InterpFields
    return _FIELDS_FUNCTION


def interp_fields(fs, obs):
    """Values of the field set `fs` (a multilinear or multicubic `Fields`) at `obs` (a sequence of N equally shaped torch CUDA
    tensors of the set's dtype): a tensor of shape `(K, *obs[0].shape)`, differentiable with respect to every tensor of `obs`.
    The table stays a constant of the graph."""
    return _fields_function().apply(fs, *obs)


def _fields_points_function():
    """The point-major field-set torch.autograd.Function, built on first use like `_function`."""
    global _FIELDS_POINTS_FUNCTION
    if _FIELDS_POINTS_FUNCTION is not None:
        return _FIELDS_POINTS_FUNCTION
    import torch

    class _InterpFieldsPoints(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fs, pts):
            shape = pts.shape
            flat = pts.detach().reshape(-1, shape[-1])
            out, jac = fs.eval_points_grad_tensors(flat)
            fs.finish()
            ctx.save_for_backward(jac)
            ctx.pts_shape = shape
            return out.reshape(tuple(shape[:-1]) + (out.shape[-1],))

        @staticmethod
        def backward(ctx, grad_out):
            (jac,) = ctx.saved_tensors  # (n, K, N)
            g = grad_out.reshape(jac.shape[0], jac.shape[1])
            # einsum("...k,...kn->...n"): pts.grad[i, d] = sum_f grad_out[i, f] * J[i, f, d], products first, then their sum
            return None, (g.unsqueeze(-1) * jac).sum(-2).reshape(ctx.pts_shape)

    _FIELDS_POINTS_FUNCTION = _InterpFieldsPoints
    return _FIELDS_POINTS_FUNCTION


def interp_fields_points(fs, pts):
    """Values of the field set `fs` (a multilinear or multicubic `Fields`) at the points `pts`, ONE torch CUDA tensor of shape
    `(..., N)` of the set's dtype: a tensor of shape `(..., K)`, differentiable with respect to `pts`.  The table stays a
    constant of the graph."""
    return _fields_points_function().apply(fs, pts)


def _lattice_function():
    """The lattice torch.autograd.Function, built on first use like `_function`."""
    global _LATTICE_FUNCTION
    if _LATTICE_FUNCTION is not None:
        return _LATTICE_FUNCTION
    import torch

    class _InterpLattice(torch.autograd.Function):
        @staticmethod
        def forward(ctx, it, *axes):
            flat = [a.detach().reshape(-1).contiguous() for a in axes]
            out, grad = it.eval_lattice_grad_tensors(flat)
            it.finish()
            ctx.save_for_backward(grad)
            ctx.axis_shapes = [a.shape for a in axes]
            return out

        @staticmethod
        def backward(ctx, grad_out):
            (grad,) = ctx.saved_tensors  # (N, *m)
            n = grad.shape[0]
            res = [None]
            for d in range(n):
                if not ctx.needs_input_grad[d + 1]:
                    res.append(None)
                    continue
                full = grad_out * grad[d]
                others = [e for e in range(n) if e != d]
                res.append((full.sum(dim=others) if others else full).reshape(ctx.axis_shapes[d]))
            return tuple(res)

    _LATTICE_FUNCTION = _InterpLattice
    return _LATTICE_FUNCTION


def interp_lattice(it, axes):
    """Value of the multilinear or multicubic interpolator `it` on the lattice axes[0] x .. x axes[N-1] (a sequence of N torch
    CUDA coordinate vectors of the handle's dtype): a tensor of shape `tuple(len(a) for a in axes)`, differentiable with
    respect to every vector of `axes`."""
    return _lattice_function().apply(it, *axes)


def _fields_lattice_function():
    """The field-set lattice torch.autograd.Function, built on first use like `_function`."""
    global _FIELDS_LATTICE_FUNCTION
    if _FIELDS_LATTICE_FUNCTION is not None:
        return _FIELDS_LATTICE_FUNCTION
    import torch

    class _InterpFieldsLattice(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fs, field_axis, *axes):
            flat = [a.detach().reshape(-1).contiguous() for a in axes]
            out, jac = fs.eval_lattice_grad_tensors(flat, field_axis=field_axis)
            fs.finish()
            ctx.save_for_backward(jac)
            ctx.axis_shapes = [a.shape for a in axes]
            ctx.field_axis = field_axis
            return out

        @staticmethod
        def backward(ctx, grad_out):
            (jac,) = ctx.saved_tensors  # (K, N, *m), or (*m, K, N)
            n = len(ctx.axis_shapes)
            res = [None, None]
            for d in range(n):
                if not ctx.needs_input_grad[d + 2]:
                    res.append(None)
                    continue
                # axes[d].grad[i] = sum over f and over every other lattice axis of grad_out * jac[f, d]
                if ctx.field_axis == 0:
                    full = grad_out * jac[:, d]
                    dims = [0] + [1 + e for e in range(n) if e != d]
                else:
                    full = grad_out * jac[..., d]
                    dims = [e for e in range(n) if e != d] + [n]
                res.append(full.sum(dim=dims).reshape(ctx.axis_shapes[d]))
            return tuple(res)

    _FIELDS_LATTICE_FUNCTION = _InterpFieldsLattice
    return _FIELDS_LATTICE_FUNCTION


def interp_fields_lattice(fs, axes, field_axis: int = 0):
    """Values of the field set `fs` (a multilinear or multicubic `Fields`) on the lattice axes[0] x .. x axes[N-1] (a sequence
    of N torch CUDA coordinate vectors of the set's dtype): a tensor of shape `(K, *m)`, or `(*m, K)` with `field_axis=-1`,
    differentiable with respect to every vector of `axes`.  The table stays a constant of the graph."""
    return _fields_lattice_function().apply(fs, field_axis, *axes)
