"""What a sampler may ask of its score network -- the one file under generators/ that probes a network attribute by name.

A score network is any callable `net(batch, conditional=False) -> AXL`; a caller's plain torch.nn.Module is a legal one.  On
top of that a network MAY carry the names below.  None is declared on ScoreNetwork (its surface is the reference's): each is
looked up on the live network at every use, never cached, so a network swapped or reconfigured on a built generator is seen.

  graph_status              int32 [1] device word the network makes in its first forward and raises MDX_STATUS_* bits in; read
                            by status_word, take_reports, clear_reports and the generator's check_status.  Absent: no reports.
  edge_chain_precision      set by the caller, and by exact_f32 for one recomputed iteration; read by reports_watched and
                            capture_key.  Absent (None): no fused edge chain, so no f16-range report.
  first_layer_table         set by the caller, and by table_off after a table report; read by reports_watched and capture_key.
                            Absent ("off"): no distance table, so no table report.
  sigma_uniform_hint        set by uniform_sigma around a forward, read by the network's forward.  Absent: a plain call.
  logits_unread_hint        set by logits_unread around a forward whose atom-type logits nobody will read; the network may then
                            return A = None and leave out the work behind the logits.  Absent: a plain call.
                            Given by the corrector steps that leave the types alone and, with ONE atom type, by the predictor
                            steps too: the MASK logit is forced to -inf, and the type update makes the same of every
                            (finite, -inf), so it runs without logits (mdx_pc_step_update, logits == NULL).  A difference in
                            failure behaviour: non-finite node features in the LAST graph layer of such a forward no longer
                            reach A (they fed the logits only; X never depended on them; the edge chain's own f16-range
                            report is untouched).  Any recorder, forward hook or overridden _get_model_predictions, and any
                            network with more than one atom type, keep the whole forward.
  capture_safe(B, N, dev)   the network's answer, asked by capture_safe.  Absent (True): the caller's use_hip_graph is believed.
  begin_f16_range_fallback  called by exact_f32 on entry.  Absent: no-op.
  adapt_f16_range           called by exact_f32 on exit.  Absent: no-op.
  force_field_parameters    the force-field wrapper's dataclass, read by capture_key.  Absent (None): no such kernel argument.

REPORTS are the bits of graph_status that ask the sampler to run an iteration again (LangevinGenerator._recover): under
exact_f32 for MDX_STATUS_EGNN_F16_RANGE, after table_off for MDX_STATUS_EGNN_TABLE.  Every other bit stays in the word for
check_status().  EGNNScoreNetwork implements all of these; ForceFieldAugmentedScoreNetwork passes them on to the network it wraps.
"""
import contextlib
import dataclasses

from .._hip import STATUS_EGNN_F16_RANGE, STATUS_EGNN_TABLE

SPLIT_F16_MODES = ("f16x3", "f16x3_32x32")
REPORTS = STATUS_EGNN_F16_RANGE | STATUS_EGNN_TABLE


def status_word(net):
    return getattr(net, "graph_status", None)


def reports_watched(net) -> bool:
    """Does the network run split-f16 kernels that can report a value beyond the f16 range, or a first-layer distance table
    that can report MDX_STATUS_EGNN_TABLE?"""
    return getattr(net, "edge_chain_precision", None) in SPLIT_F16_MODES or getattr(net, "first_layer_table", "off") != "off"


def take_reports(net) -> int:
    """Read the network's status word (a host synchronisation) and clear those of its REPORTS bits that were set (other bits
    stay for check_status())."""
    status = status_word(net)
    word = 0 if status is None else int(status.item()) & REPORTS
    if word:
        status.bitwise_and_(~REPORTS)
    return word


def clear_reports(net):
    """No host read.  A report bit left in the network's word by something that was not an iteration of the loop (the warm-up
    iterations before a capture, a caller stepping by hand, iterations a rollback dropped) must not be read as the next
    iteration's report."""
    status = status_word(net)
    if status is not None and reports_watched(net):
        status.bitwise_and_(~REPORTS)


def capture_safe(net, batch: int, atoms: int, device) -> bool:
    """A network may say that its forward on this batch shape needs a host synchronisation (EGNNScoreNetwork with a radius
    graph whose layers do not all run the fused edge chain, or whose capacity-sized edge list does not fit)."""
    ask = getattr(net, "capture_safe", None)
    return True if ask is None else bool(ask(batch, atoms, device))


@contextlib.contextmanager
def uniform_sigma(net):
    """Around a forward whose batch holds ONE sigma (the sampler fills it itself): the network may run its first graph layer
    on a distance grid."""
    if not hasattr(net, "sigma_uniform_hint"):
        yield
        return
    net.sigma_uniform_hint = True
    try:
        yield
    finally:
        net.sigma_uniform_hint = False


def outputs_watched(net) -> bool:
    """Does a forward hook -- on the network, on a module inside it, or torch's global ones -- see outputs of the forward?  Then
    the forward is run whole (no logits_unread)."""
    import torch.nn.modules.module as m
    if m._global_forward_hooks:
        return True
    modules = net.modules() if hasattr(net, "modules") else ()
    return any(getattr(mod, "_forward_hooks", None) for mod in modules)


@contextlib.contextmanager
def logits_unread(net):
    """Around a forward whose atom-type logits nobody reads (a corrector step that does not update the types, or any step with
    one atom type, with nothing recording or inspecting the predictions): the network may return A = None."""
    if not hasattr(net, "logits_unread_hint"):
        yield
        return
    net.logits_unread_hint = True
    try:
        yield
    finally:
        net.logits_unread_hint = False


@contextlib.contextmanager
def exact_f32(net):
    """The exact-f32 pass after an f16-range report.  On entry the network forgets the activation maxima earlier f32 launches
    left, so that they describe THIS pass; on exit its precision is put back and it derives per-layer activation exponents
    for its split-f16 kernels from those maxima (a layer that runs hot does not send every following iteration here)."""
    precision = net.edge_chain_precision
    getattr(net, "begin_f16_range_fallback", lambda: None)()
    net.edge_chain_precision = "f32"
    try:
        yield
    finally:
        net.edge_chain_precision = precision
        getattr(net, "adapt_f16_range", lambda: None)()


def table_off(net):
    """After a table report: the network's first layer goes back to the per-edge chain for the rest of the process."""
    net.first_layer_table = "off"


def capture_key(net) -> tuple:
    """What a captured forward depends on besides the parameters: the arithmetic mode, the table setting, and the force-field
    wrapper's cutoff and strength (kernel arguments: their values, not the mutable object)."""
    force_field = getattr(net, "force_field_parameters", None)
    return (getattr(net, "edge_chain_precision", None), getattr(net, "first_layer_table", None),
            None if force_field is None else dataclasses.astuple(force_field))
