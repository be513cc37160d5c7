"""What a trainer and the field agree on.  NGP and implicit_mask each carry a FieldLink as `self.link`: NGPTrainer fills it,
the field's autograd nodes (networks._FieldFn, implicit_mask._MaskFieldFn) read it.  It is no nn.Module and holds no
parameter or buffer, so it never shows in state_dict().  Every default means "no trainer": gradients go through
autograd, launches on the field's per-device default streams, nothing to wait for."""
from ._lib import call


class FieldLink:
    __slots__ = ("grad_sinks", "side_stream", "heads_stream", "params_ready", "rgb_params_ready", "acc_zeroed",
                 "norm_acc", "hits", "ok")

    def __init__(self):
        # name -> view of the trainer's flat gradient: the backward accumulates straight into it and autograd gets None.
        # NGP: W1 b1 W2 b2 rgb_p nrm_p sem_p embedding_a; implicit_mask: table W1 b1 W2 b2
        self.grad_sinks = {}
        # the backward's table scatters / the forward's two 32-wide heads; None = the per-device default stream
        self.side_stream = self.heads_stream = None
        # The optimizer's sweep in two pieces, [density table | MLPs] and the colour table (77 % of the bytes): whatever reads
        # parameters waits for the piece it needs.  Anything with .wait(): a HIP event (one GPU: clip + Adam on the optimizer
        # stream) or the handle of an async all-gather of the updated shards (sharded optimizer).
        self.params_ready = self.rgb_params_ready = None
        self.acc_zeroed = None     # the trainer clears its norm accumulators behind the Adam launches
        # Clip from a norm bound (ngp_clip_decide): ||table gradient|| <= ||W1||_F ||W2||_F sum_s ||dz2[s]||.  norm_acc takes
        # the two sums (slot 0: rgb_net, 1: density head) on a bound step only; the bound holds when both MLP backwards
        # noted theirs (hits == 2) and nothing else added to a table gradient (ok).
        self.norm_acc = None
        self.hits, self.ok = 0, True

    def take_param_events(self):
        """-> (MLP piece, colour piece), both cleared: the caller makes each of its streams wait where it first reads"""
        evs = self.params_ready, self.rgb_params_ready
        self.params_ready = self.rgb_params_ready = None
        return evs

    def join_params(self, rgb_table=True):
        """the current stream waits for the sweep (rgb_table=False: for its first piece only); the events stay in place, the
        field waits for them as well"""
        for ev in (self.params_ready, self.rgb_params_ready if rgb_table else None):
            if ev is not None:
                ev.wait()

    def wait_params(self, rgb_table=True):
        """join_params, and what was waited for is cleared (rgb_table=False leaves the colour piece pending)"""
        self.join_params(rgb_table)
        self.params_ready = None
        if rgb_table:
            self.rgb_params_ready = None

    def take_acc_zeroed(self):
        ev, self.acc_zeroed = self.acc_zeroed, None
        return ev

    def begin_bound_step(self, norm_acc):
        """before a step's backward; norm_acc: the trainer's accumulator on a bound step, else None"""
        self.norm_acc = norm_acc
        self.hits, self.ok = 0, True

    def bound_note(self, st, slot, n_out, n):
        """accumulate sum_s ||dz2[s]|| of the MLP whose backward `st` (a networks._Mlp2Bwd) is"""
        if self.norm_acc is None:
            return
        if not st.fused:
            self.ok = False
            return
        if not st.norm_noted:      # (the elementwise stage adds the sum itself when it is handed the accumulator)
            call("row_norm_sum", st.dz2, n_out, n, n_out, self.norm_acc[slot:slot + 1])
        self.hits += 1

    def bound_spoiled(self):
        self.ok = False
