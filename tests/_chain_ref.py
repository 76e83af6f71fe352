"""The causal stages of the post-processing chain on the host, by the library's own host statements (ptts_compress_apply, the blocked DC block,
ptts_eq_apply, ptts_dsp_apply's fades), in the chain's order: what the windows of a streamed joined call must reproduce bit for bit.  Shared by
test_gpu_dsp_windows.py and test_gpu_join_stream.py."""
import numpy as np

TILE = 1920


class Chain:
    """compressor: a CompressorOpts or None; eq: sections for runtime.Eq or None."""

    def __init__(self, pkg, compressor=None, dc_block=False, eq=None, fade_in_ms=0.0, fade_out_ms=0.0):
        self.pkg, self.rt = pkg, pkg.runtime
        self.compressor, self.dc_block, self.fade_in_ms, self.fade_out_ms = compressor, dc_block, fade_in_ms, fade_out_ms
        self.eq = self.rt.Eq(eq) if eq else None
        self.opts = self.rt._dsp_opts(pkg.RuntimeGenerateConfig(compressor=compressor, dc_block=dc_block, eq=self.eq, fade_in_ms=fade_in_ms,
                                                                fade_out_ms=fade_out_ms))

    def host(self, x):
        """The whole chain over one row, on the host."""
        rt = self.rt
        y = np.array(x, np.float32, copy=True)
        if y.size == 0:
            return y
        if self.compressor is not None:
            y = rt.compress_apply(self.compressor, y)
        if self.dc_block:
            y = rt.dsp_blocked_host(y)
        if self.eq is not None:
            y = self.eq.apply(y)
        if self.fade_in_ms > 0 or self.fade_out_ms > 0:
            y = rt.dsp_apply(y, fade_in_ms=self.fade_in_ms, fade_out_ms=self.fade_out_ms)
        return y

    def stateless(self, x, cuts):
        """The chain applied to each window on its own and concatenated: what windows WITHOUT carried state would give."""
        edges = [0] + [c for c in cuts if c < x.size] + [x.size]
        return np.concatenate([self.host(x[a:b]) for a, b in zip(edges, edges[1:])]) if x.size else np.array(x, np.float32)


def fade_out_samples(ms):
    return int(np.float64(ms) / np.float64(1000.0) * np.float64(24000.0)) if ms > 0 else 0


def legal_cuts(cuts, lengths, fade_out_ms):
    """The cuts that deliver no part of a row's fade out: none with c < n and c > n - Fo for a row of n samples."""
    fo = fade_out_samples(fade_out_ms)
    return [c for c in cuts if not any(c < n and c > n - fo for n in lengths)]
