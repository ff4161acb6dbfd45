"""What the autograd Functions of the model classes share: the end of a property's forward pass, the scatter of its backward
pass, the stability flag of a bubble / dew solution, and the bookkeeping of the state-function Functions.  A Function keeps
what is its own: which solve and which Jacobian it calls.  A column table holds (first column, columns, shape) per input."""
from . import native


def finish(ctx, out_device, values, nans, *flags):
    """End of a property's forward: values, then nans and further flags (non-differentiable), on the caller's device."""
    flags = [t.to(out_device) for t in (nans, *flags)]
    ctx.mark_non_differentiable(*flags)
    return [v.to(out_device) for v in values] + flags


def scatter(comp, jac, g, table, needs, devices):
    """Backward of a property: per needed input g_j * jac[j, columns] in the row of the j-th kept row (zeros in dropped rows,
    one kernel each), on that input's device.  g None: jac carries the upstream gradients already."""
    g = None if g is None else g.to(comp.device).contiguous()
    return [comp.expand(jac, g, col0, ncol).view(shape).to(dev) if need else None
            for (col0, ncol, shape), need, dev in zip(table, needs, devices)]


def stable_at_solution(comp, rho4, dew, stability):
    """bool [n_ok], aligned with the value: the specified phase (liquid for bubble, vapour for dew) at the converged solution
    passes `stability(feed densities [n_ok, 2])` (native.mix_stability / gc_stability on the compacted rows)."""
    rho4 = comp.gather(rho4)
    return stability(rho4[:, 0:2] if dew else rho4[:, 2:4])["status"] == 0


def save_state(ctx, inputs, saved, outputs):
    """Forward of a state function: keeps the prepared inputs for the VJP kernel and the devices of the caller's tensors;
    outputs on the device of the first input.  Unused outputs reach backward as None (no zero tensors are made)."""
    ctx.save_for_backward(*saved)
    ctx.set_materialize_grads(False)
    ctx.in_devices = tuple(x.device for x in inputs)
    return tuple(o.to(ctx.in_devices[0]) for o in outputs)


def split(packed, table, needs, devices):
    """Backward of a state function: the needed inputs' column ranges of the packed gradient [n, k], each on its input's device."""
    return tuple(packed[:, col0:col0 + ncol].contiguous().view(shape).to(dev) if need else None
                 for (col0, ncol, shape), need, dev in zip(table, needs, devices))


class Reducible:
    """`reduce` of the model classes; a class brings `_reduce(comp)` and the device it computes on."""

    def reduce(self, nans):
        """Drop the rows flagged in ``nans`` from the model."""
        self._reduce(native.Compaction(nans.to(self._compute_device())))

    def _compute_device(self):
        return native._device_of(self._par)
