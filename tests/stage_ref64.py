"""Float64 restatement of each model stage, for judging the fp32 kernels one stage at a time.

TEST INFRASTRUCTURE ONLY.  Every function takes the input of its stage -- on the GPU tests, the GPU's own output of the stage
before (the debug taps) -- and returns the stage's output in float64 on the input's device, so that a stage's error is its own
and not the sum of everything upstream.  Weights are sdfa_oracle.Oracle's folded tensors (as oracle/torch_oracle.py takes
them) and the operator order is TorchOracle.encoder / forward; nothing here calls a project kernel.  The LSTM recurrences are
written out (gate order i, f, g, o) and the convolutions along frequency are sums of shifted matrix products, so every
operator is a plain float64 matmul / elementwise op on any device.

Pinned to the reference project's fixtures by tests/test_stage_ref64_cpu.py.

Both output heads: `head="dgrad"` (scale / rotation regressors, two PCA inversions interleaved) and `head="offsets"` (three FCs to
59 coefficients, one PCA inversion to 15,069 columns).

The keyword arguments `drop_h`, `stale`, `drop_mean` and `bf16_basis` perturb the reference the way a subtle kernel bug would (a
step that loses its recurrent input, a work unit that reads the wrong time step, an output column without its mean term, a PCA
expansion whose basis keeps its bf16 high term only); the GPU tests use them to show that their bounds catch such a bug.
"""
import numpy as np
import torch

import sdfa_oracle as O

F64 = torch.float64


class StageRef64:
    def __init__(self, state_dict, device="cpu", head="dgrad"):
        assert head in ("dgrad", "offsets")
        o = O.Oracle(state_dict, head)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=F64)
        self.device = device
        self.head = head
        self.w_conv = [tuple(t(x) for x in c) for c in o.conv]                    # w (co, ci, kf), b, bn scale, bn shift
        self.w_freq = [(t(wi), t(wh), t(b)) for wi, wh, b in o.freq]               # bias_ih + bias_hh folded
        self.freq_proj = tuple(t(x) for x in o.freq_proj)
        self.w_bilstm = [[(t(wi), t(wh)) for wi, wh, _ in layer] for layer in o.bilstm]
        self.w_attn = {k: t(v) for k, v in o.attn.items()}
        self.trunk = [tuple(t(x) for x in wb) for wb in o.trunk]                 # dgrad: _layers.0; offsets: _layers.0 .. 2
        if head == "dgrad":
            self.scale = [tuple(t(x) for x in wb) for wb in o.scale]
            self.rotat = [tuple(t(x) for x in wb) for wb in o.rotat]
            self.pca_s = tuple(t(x) for x in o.pca_s)                            # compT (59856, 85), means (59856,)
            self.pca_r = tuple(t(x) for x in o.pca_r)                            # compT (29928, 180), means (29928,)
        else:
            self.pca = tuple(t(x) for x in o.pca)                                # compT (15069, 59), means (15069,)

    def _in(self, x):
        return torch.as_tensor(x).to(device=self.device, dtype=F64)

    # ------------------------------------------------------------------ stages
    @torch.no_grad()
    def conv_stack(self, audio_feat):
        """audio_feat (n, 64, 128, 3) -> conv3 (n, 64, 32, 64): three Conv2d (kf, 1) 'same' along frequency, LeakyReLU(0.2), then
        the eval BatchNorm; max-pool (2, 1) after the first two."""
        x = self._in(audio_feat).permute(0, 3, 2, 1)                              # (n, 3, 128, 64)
        for i, (w, b, sc, sh) in enumerate(self.w_conv):
            kf = w.shape[2]
            Fq = x.shape[2]
            xp = torch.nn.functional.pad(x, (0, 0, kf // 2, kf // 2))
            y = sum(torch.einsum("oc,ncft->noft", w[:, :, d], xp[:, :, d:d + Fq, :]) for d in range(kf))
            y = torch.nn.functional.leaky_relu(y + b.view(1, -1, 1, 1), 0.2) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
            x = torch.maximum(y[:, :, 0::2], y[:, :, 1::2]) if i < 2 else y
        return x

    @staticmethod
    def _lstm_dir(gx, w_hh, reverse, drop_step=None):
        """One direction of torch.nn.LSTM from its input projection gx (B, S, 4H) -> (B, S, H).  drop_step: that step's gates
        get no recurrent term."""
        B, S, G = gx.shape
        H = G // 4
        h = gx.new_zeros(B, H)
        c = gx.new_zeros(B, H)
        out = gx.new_empty(B, S, H)
        for t in (range(S - 1, -1, -1) if reverse else range(S)):
            g = gx[:, t] if t == drop_step else gx[:, t] + h @ w_hh.T
            i = torch.sigmoid(g[:, :H]); f = torch.sigmoid(g[:, H:2 * H])
            gg = torch.tanh(g[:, 2 * H:3 * H]); o = torch.sigmoid(g[:, 3 * H:])
            c = f * c + i * gg
            h = o * torch.tanh(c)
            out[:, t] = h
        return out

    @torch.no_grad()
    def freq(self, conv3, chunk=256):
        """conv3 (n, 64, 32, 64) -> Z (n, 256, 64): the frequency BiLSTM (with bias) over the 32 bands of every (frame, time step),
        then Linear(8192 -> 256).  Layout of the debug tap: channel-major."""
        x = self._in(conv3)
        n = x.shape[0]
        out = x.new_empty(n, 256, 64)
        w, b = self.freq_proj
        for f0 in range(0, n, chunk):
            xs = x[f0:f0 + chunk]
            m = xs.shape[0]
            seq = xs.permute(0, 3, 2, 1).reshape(m * 64, 32, 64)
            h = torch.cat([self._lstm_dir(seq @ wi.T + bb, wh, reverse=d == 1) for d, (wi, wh, bb) in enumerate(self.w_freq)], -1)
            z = (h.reshape(m * 64, 32 * 256) @ w.T + b).reshape(m, 64, 256)
            out[f0:f0 + m] = z.transpose(1, 2)
        return out

    @torch.no_grad()
    def bilstm(self, Z, drop_h=None, chunk=2048):
        """Z (n, 256, 64) -> H1 (n, 64, 512): two bidirectional layers without bias.  drop_h = (layer, direction, step)."""
        x = self._in(Z)
        n = x.shape[0]
        out = x.new_empty(n, 64, 512)
        for f0 in range(0, n, chunk):
            y = x[f0:f0 + chunk].transpose(1, 2)
            for l, layer in enumerate(self.w_bilstm):
                y = torch.cat([self._lstm_dir(y @ wi.T, wh, reverse=d == 1,
                                              drop_step=drop_h[2] if drop_h and drop_h[:2] == (l, d) else None)
                               for d, (wi, wh) in enumerate(layer)], -1)
            out[f0:f0 + y.shape[0]] = y
        return out

    @torch.no_grad()
    def attention(self, H1, stale=None, chunk=4096):
        """H1 (n, 64, 512) -> z (n, 512), align (n, 64): Conv1d query over time steps 31..33, additive attention over all 64
        steps, softmax, context.  stale = (frame0, t): frames frame0 .. frame0+15 read step t+1's keys and values in place of t's."""
        x = self._in(H1)
        a = self.w_attn
        n = x.shape[0]
        z, align = x.new_empty(n, 512), x.new_empty(n, 64)
        for f0 in range(0, n, chunk):
            h = x[f0:f0 + chunk]
            q = torch.einsum("ock,nkc->no", a["conv"], h[:, 31:34])
            hk = h
            if stale is not None and f0 <= stale[0] < f0 + chunk:
                u, t = stale[0] - f0, stale[1]
                hk = h.clone()
                hk[u:u + 16, t] = h[u:u + 16, t + 1]
            s = torch.tanh((q @ a["wq"].T)[:, None, :] + hk @ a["wk"].T + a["b"]) @ a["v"]
            al = torch.softmax(s, -1)
            z[f0:f0 + chunk] = torch.einsum("nt,ntc->nc", al, hk)
            align[f0:f0 + chunk] = al
        return z, align

    @torch.no_grad()
    def regress(self, z, speaker_id):
        """z (n, 512), speaker ids (n,) -> dgrad: coef (n, 265) = [scale coefficients (85) | rotation coefficients (180)];
        offsets: coef (n, 59), Linear + LeakyReLU(0.2) over [z | speaker one-hot], Linear + tanh, Linear."""
        z = self._in(z)
        spk = torch.as_tensor(speaker_id).to(device=self.device, dtype=torch.int64).reshape(-1)
        c = torch.nn.functional.one_hot(spk, 8).to(F64)
        fc = lambda x, wb: x @ wb[0].T + wb[1]
        lrelu = lambda y: torch.nn.functional.leaky_relu(y, 0.2)
        if self.head == "offsets":
            return fc(torch.tanh(fc(lrelu(fc(torch.cat([z, c], -1), self.trunk[0])), self.trunk[1])), self.trunk[2])
        hc = torch.cat([lrelu(fc(torch.cat([z, c], -1), self.trunk[0])), c], -1)
        cs = fc(torch.tanh(fc(lrelu(fc(hc, self.scale[0])), self.scale[1])), self.scale[2])
        cr = fc(torch.tanh(fc(lrelu(fc(hc, self.rotat[0])), self.rotat[1])), self.rotat[2])
        return torch.cat([cs, cr], -1)

    @torch.no_grad()
    def expand(self, coef, drop_mean=None, bf16_basis=False):
        """dgrad: coef (n, 265) -> rows (n, 89784): both PCA inversions, interleaved per triangle as (6 scale, 3 rotation) values;
        offsets: coef (n, 59) -> rows (n, 15069), one PCA inversion.  drop_mean: a column of the rows whose mean term is left out.
        bf16_basis: the basis rounded to bf16 (its high term alone: what a split-bf16 expansion computes once it loses the low terms
        of the basis); the means and the coefficients stay as they are."""
        coef = self._in(coef)
        n = coef.shape[0]
        basis = (lambda b: b.bfloat16().double()) if bf16_basis else (lambda b: b)
        if self.head == "offsets":
            rows = coef @ basis(self.pca[0]).T + self.pca[1]
        else:
            s = (coef[:, :85] @ basis(self.pca_s[0]).T + self.pca_s[1]).reshape(n, -1, 6)
            r = (coef[:, 85:] @ basis(self.pca_r[0]).T + self.pca_r[1]).reshape(n, -1, 3)
            rows = torch.cat([s, r], -1).reshape(n, -1)
        if drop_mean is not None:
            rows[:, drop_mean] -= self.row_means()[drop_mean]
        return rows

    def row_means(self):
        """The mean term of every output column, in the rows' layout."""
        if self.head == "offsets":
            return self.pca[1]
        return torch.cat([self.pca_s[1].reshape(-1, 6), self.pca_r[1].reshape(-1, 3)], -1).reshape(-1)
