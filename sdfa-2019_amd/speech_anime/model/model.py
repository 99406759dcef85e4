"""SpeechDrivenAnimation / SaberSpeechDrivenAnimation -- inference surface of speech_anime/model/model.py.

Same method names, arguments and result layouts as the reference; the arithmetic is libsdfa_hip.so.
Not mirrored (out of scope): the encoder's backward and with it the full training loop, TensorBoard hooks,
titles and the multi-source grid of the evaluate video.  The regressor head alone trains with the encoder frozen: train_step,
fit_head, head_state_dict and commit_head (sdfa_amd.headtrain).  get_loss is the training objective on PCA coefficients
(sdfa_amd.objective); its validation scalars over whole clips are validate() (sdfa_amd.score).  evaluate() writes the dgrad track, .obj files with a template mesh and, with save_video, an
.avi rendered on the GPU (sdfa_amd.render, speech_anime.video).
"""
import os
from copy import deepcopy

import numpy as np
import torch

from sdfa_amd.engine import Engine
from sdfa_amd import weights as _weights
from sdfa_amd import ops as _ops
from ..datasets import DatasetSlidingWindow
from .. import audio as _audio
from .. import stream as _stream


class SpeechDrivenAnimation:
    """audio_feat -> anime_feat model (model.py:18-45)."""

    def __init__(self, hparams, load_pca=False):
        self.hp = hparams
        self._face_type = hparams.model.face_data_type
        self._engine = None

    def load_state_dict(self, state_dict, strict=True):
        head = _weights.head_of(state_dict)
        want = "dgrad" if self._face_type == "dgrad_3d" else "offsets"
        if head != want:
            raise RuntimeError(f"checkpoint holds a '{head}' output module but hparams.model.face_data_type = {self._face_type}")
        self._engine = Engine(state_dict, device=self.hp.get("device", "cuda:0") or "cuda:0",
                              precision=self.hp.get("precision", "fp32") or "fp32", strict=strict)
        # weakly registered: dropping this object frees the engine (weights + workspace); anonymous keys come from a counter
        self._key = _ops.register_model(self.hp.get("model_key") or None, self._engine)
        return self

    def eval(self):
        return self

    def __call__(self, *a, **k):
        return self.forward(*a, **k)

    @torch.no_grad()
    def forward(self, audio_feat, speaker_id, align_dict=None, latent_dict=None):
        """(N,64,128,3) f32, (N,) int64 -> ((scale (N,1,9976,6), rotat (N,1,9976,3)), z_audio (N,1,512)); offsets head:
        (pred (N,1,15069), z_audio).  A dict `align_dict` receives {"audio_encoder10": (N,1,64)} (layers/__init__.py:98-99)."""
        if self._engine is None:
            raise RuntimeError("no weights loaded: call load_state_dict first")
        eng = self._engine
        x = audio_feat.to(device=eng.device, dtype=torch.float32)
        n = x.shape[0]
        # the arithmetic is two dispatcher-visible PyTorch-ROCm custom ops over the C ABI (sdfa_amd/ops.py)
        z, align = torch.ops.sdfa.encoder(x.contiguous(), self._key)
        if isinstance(align_dict, dict):
            align_dict["audio_encoder10"] = align.view(n, 1, 64)
        out = torch.ops.sdfa.regress(z, speaker_id.to(eng.device), self._key)
        z_audio = z.view(n, 1, 512)
        if self._face_type == "dgrad_3d":
            tri = out.view(n, 1, -1, 9)
            return (tri[..., :6], tri[..., 6:]), z_audio      # views into the interleaved [6 | 3] rows
        return out.view(n, 1, -1), z_audio


class SaberSpeechDrivenAnimation:
    """Handles evaluation (model.py:48-489, inference half)."""

    def __init__(self, hparams, trainset=None, validset=None, load_pca=True):
        self.hp = hparams
        self.trainset, self.validset = trainset, validset
        self._model = SpeechDrivenAnimation(hparams, load_pca)
        self._face_type = hparams.model.face_data_type
        self._pred_type = hparams.model.prediction_type
        self._speakers_dict = deepcopy(dict(hparams.dataset_anime.speakers))
        self._emotions_dict = deepcopy(dict(hparams.dataset_anime.emotions))
        self.current_epoch = 0
        self.on_gpu = True
        self.training = False
        self._loss_scalers = dict()      # DynamicLossScaler by the reference's name (dyn_p_scale, ...), made on first use

    # ---- weights ------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict=True):
        self._model.load_state_dict(state_dict, strict)
        self._signal_cache = None
        DatasetSlidingWindow.use_engine(self._model._engine)
        return self

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        """Only get_loss looks at it: in training the DynamicLossScalers update."""
        self.training = bool(mode)
        return self

    def clear_signal_cache(self):
        """Drop the one-entry signal -> z cache of generate_animation (frees z and the kept features on the device)."""
        self._signal_cache = None

    def __call__(self, batch):
        return self.forward(batch)

    # ---- model.py:79-107 ----------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, batch):
        align_dict, latent_dict = dict(), dict()
        preds, condition = self._model(batch["audio_feat"], batch["speaker_id"], align_dict=align_dict, latent_dict=latent_dict)
        pred_dict = dict()
        if self._face_type == "dgrad_3d":
            assert len(preds) == 2
            pred_dict["dgrad_3d_scale"], pred_dict["dgrad_3d_rotat"] = preds
        else:
            # the reference asserts len(preds) == 1 on a bare tensor here (only true for batch 1)
            pred_dict[self._face_type] = preds
        return dict(prediction=pred_dict, condition=condition, align_dict=align_dict, latent_dict=latent_dict)

    # ---- model.py:225-259 ---------------------------------------------------------------------
    def data_to_anime_feat(self, tensor_dict, is_prediction):
        if self._face_type == "dgrad_3d":
            scale, rotat = tensor_dict["dgrad_3d_scale"], tensor_dict["dgrad_3d_rotat"]
            data = torch.cat((scale.reshape(*scale.shape[:-1], -1, 6), rotat.reshape(*rotat.shape[:-1], -1, 3)), dim=-1)
            return data.reshape(*data.shape[:-2], -1)
        return tensor_dict[self._face_type]

    # ---- model.py:261-330 ---------------------------------------------------------------------
    def _train_losses(self, coef, truth, weight):
        """(ps, ms, pr, mr) as a differentiable float32 [4] on the device (sdfa_amd/ops.py)."""
        return torch.ops.sdfa.train_losses(coef, truth, weight, self._model._key)

    def enable_training_objective(self, state_dict):
        """Put the head's plain PCA bases (`state_dict`: the one given to load_state_dict, or a sdfa_amd.pca result under the
        reference's names) on the device, once; get_loss needs it.  Inference-only use never pays for it."""
        from sdfa_amd.objective import attach_bases
        if self._model._engine is None:
            raise RuntimeError("no weights loaded: call load_state_dict first")
        attach_bases(self._model._engine, state_dict)
        return self

    def _scaler(self, name):
        from sdfa_amd.objective import DynamicLossScaler
        if name not in self._loss_scalers:
            self._loss_scalers[name] = DynamicLossScaler()
        return self._loss_scalers[name]

    def get_loss(self, pred_dict, batch):
        """The reference's objective for prediction_type "face_data" with a frozen PCA (pca_trainable = False), taken on
        the PCA coefficients: pred_dict["prediction"] holds them under "dgrad_3d_coef" (N, Ks + Kr; scale first, as
        sdfa::regress_coef writes them) or "{face_data_type}_coef" (N, K) for the offsets head; `batch` is what
        DatasetSlidingWindow.train_batch returns ("face_data" (2B, W), "audio_feat", and the weights named by
        hparams.loss.anime_loss_weight -- None means ones); enable_training_objective(state_dict) must have been called.
        Returns (losses, scalars) with the reference's keys:
        dyn_ps / dyn_ms / dyn_pr / dyn_mr (hparams.loss.dynamic_scalar, the default) or loss_ps / ..., dyn_ploss / dyn_mloss or
        loss_ploss / loss_mloss for the offsets head, each times ploss_scale / mloss_scale; scalar_ps, scalar_ms, scalar_pr,
        scalar_mr, scalar_ploss, scalar_mloss.  `losses` are differentiable device scalars whose sum is the objective; their
        backward reaches the coefficients.  The four values are read back once (the reference reads each with .item()).
        ELoss is absent: this model emits no evector."""
        hp = self.hp.get("loss") or {}
        dynamic = bool(hp.get("dynamic_scalar", True))
        p_scale, m_scale = float(hp.get("ploss_scale", 1)), float(hp.get("mloss_scale", 1))
        dgrad = self._face_type == "dgrad_3d"
        coef = pred_dict["prediction"]["dgrad_3d_coef" if dgrad else f"{self._face_type}_coef"]
        truth = batch["face_data"]
        wkey = hp.get("anime_loss_weight")
        weight = batch[wkey] if wkey is not None else torch.ones(coef.shape[0], dtype=torch.float32, device=coef.device)
        loss4 = self._train_losses(coef, truth, weight)
        vals = [float(v) for v in loss4.detach().cpu().tolist()]
        losses, scalars = dict(), dict()
        if dgrad:
            terms = (("ps", "dyn_p_scale", p_scale), ("ms", "dyn_m_scale", m_scale), ("pr", "dyn_p_rotat", p_scale), ("mr", "dyn_m_rotat", m_scale))
            for i, (name, _, _) in enumerate(terms):
                scalars["scalar_" + name] = vals[i]
            scalars["scalar_ploss"] = scalars["scalar_ps"] + scalars["scalar_pr"]
            scalars["scalar_mloss"] = scalars["scalar_ms"] + scalars["scalar_mr"]
        else:
            terms = (("ploss", "dyn_p", p_scale), ("mloss", "dyn_m", m_scale))
            scalars["scalar_ploss"], scalars["scalar_mloss"] = vals[0], vals[1]
        for i, (name, scaler, mult) in enumerate(terms):
            if dynamic:
                sc = self._scaler(scaler)
                if self.training:
                    sc.update(vals[i])
                losses["dyn_" + name] = loss4[i] / sc.scale * mult
            else:
                losses["loss_" + name] = loss4[i] * mult
        return losses, scalars

    # ---- fine-tuning the regressor head: model.py:109-113, saber_model.py:46-57, trainer.py:266-320 ----
    def _head_optimizer_args(self):
        """torch.optim.Adam's arguments from hparams.optim as saber_model.configure_optimizers reads them (default: the
        model configurations' Adam(lr=1e-4, weight_decay=0)).  What the reference's configurations allow and this does not
        build is refused by name."""
        hp = self.hp
        optim = hp.get("optim") or {}
        args = dict(optim.get("args") or {})
        args.pop("__entirety__", None)
        trainer = hp.get("trainer") or {}
        refusals = (
            (optim.get("name", "Adam") != "Adam", f"optim.name = {optim.get('name')!r}: only Adam is built"),
            (float(args.get("weight_decay", 0) or 0) != 0.0, f"optim.args.weight_decay = {args.get('weight_decay')!r}: weight decay is not built"),
            (bool(args.get("amsgrad", False)), "optim.args.amsgrad: not built"),
            (optim.get("lr_scheduler") is not None, "optim.lr_scheduler: schedulers are not built"),
            (not hp.model.get("weight_norm", True), "model.weight_norm = False: the head is trained through its weight norm only"),
            (trainer.get("max_grad_clip") is not None or trainer.get("max_grad_norm") is not None, "trainer.max_grad_clip / max_grad_norm: gradient clipping is not built"),
            (int(trainer.get("grad_acc_steps", 1) or 1) > 1, f"trainer.grad_acc_steps = {trainer.get('grad_acc_steps')!r}: gradient accumulation is not built"),
            (bool(((hp.model.get("output") or {}).get("pca_trainable", False))), "model.output.pca_trainable: a trainable PCA is not built"),
        )
        for bad, why in refusals:
            if bad:
                raise NotImplementedError("head training: " + why)
        unknown = set(args) - {"lr", "betas", "eps", "weight_decay", "amsgrad"}
        if unknown:
            raise NotImplementedError(f"head training: optim.args {sorted(unknown)} are not built")
        return dict(lr=float(args.get("lr", 1e-4)), betas=tuple(args.get("betas", (0.9, 0.999))), eps=float(args.get("eps", 1e-8)))

    def enable_head_training(self, state_dict, attention=False, bilstm_top=False, bilstm_dropout=0.0, bilstm_bottom=False, freq_lstm=False,
                             conv_stack=False):
        """Make the regressor head of `state_dict` (the one given to load_state_dict: weight_g / weight_v / bias under the
        reference's names) trainable on the device, with the encoder frozen: a sdfa_amd.headtrain.HeadTrainer with the
        reference's optimiser, and the PCA bases for get_loss.  The finalised inference engine stays read-only; commit_head()
        makes a fresh one from the tuned head.

        attention=True also trains the Bahdanau attention layer (layer 10 of the audio encoder) through a
        sdfa_amd.attntrain.AttnTrainer with the same optimiser arguments and the same refusals: "attention + head, recurrent
        stack frozen".  The recurrent stack runs in its inference form, without dropout.

        bilstm_top=True (with attention=True) also trains the top layer of the BiLSTM (layer 1 of layer 9 of the audio encoder;
        DESIGN.md section 18) through a sdfa_amd.lstmtrain.LstmTrainer: the frozen stack ends at the layer-0 output, and the
        attention layer's dH flows into the BiLSTM layer's backward.  bilstm_dropout = p > 0 is nn.LSTM's inter-layer dropout in
        training mode (the reference trains with 0.1): the layer-0 output is multiplied by a Bernoulli keep mask over (1 - p),
        drawn from self._train_generator, a torch.Generator on the device the caller may seed.  The default 0.0 is the
        inference form, as above.

        bilstm_bottom=True (with bilstm_top=True) also trains the bottom layer of the BiLSTM through a
        second LstmTrainer(layer=0): the frozen stack ends at the frequency projection (torch.ops.sdfa.encoder_x0), the top
        layer's dX flows through the keep mask into the bottom layer's backward, and everything above the frequency LSTM trains.

        freq_lstm=True (with bilstm_bottom=True) also trains the frequency LSTM and its projection (layer 6 of the audio encoder;
        DESIGN.md section 21) through a sdfa_amd.freqtrain.FreqTrainer: the frozen stack ends at the conv stack
        (torch.ops.sdfa.encoder_conv), the bottom layer forms dX0, and everything above the conv stack trains.

        conv_stack=True (with freq_lstm=True) also trains the conv stack (layers 1, 3 and 5 of the audio encoder; DESIGN.md section
        22) through a sdfa_amd.convtrain.ConvTrainer: the frequency LSTM forms dC, every parameter the reference's optimiser holds
        trains, and the frozen engine no longer runs inside a training step.  BatchNorm keeps its running statistics (the
        inference form, as bilstm_dropout=0.0 is): the reference's train() mode, batch statistics and moving running ones, is
        not built."""
        from sdfa_amd.headtrain import HeadTrainer, register_trainer
        if conv_stack and not freq_lstm:
            raise NotImplementedError("head training: conv_stack=True needs freq_lstm=True: the conv stack is trained through the frequency LSTM's dC")
        if freq_lstm and not bilstm_bottom:
            raise NotImplementedError("head training: freq_lstm=True needs bilstm_bottom=True: the frequency LSTM is trained through the bottom layer's dX")
        if bilstm_bottom and not bilstm_top:
            raise NotImplementedError("head training: bilstm_bottom=True needs bilstm_top=True: the bottom layer is trained through the top layer's dX")
        if bilstm_top and not attention:
            raise NotImplementedError("head training: bilstm_top=True needs attention=True: the BiLSTM layer is trained through the attention layer's dH")
        if not 0.0 <= float(bilstm_dropout) < 1.0:
            raise ValueError(f"head training: bilstm_dropout = {bilstm_dropout!r} outside [0, 1)")
        if float(bilstm_dropout) > 0.0 and not bilstm_top:
            raise NotImplementedError("head training: bilstm_dropout needs bilstm_top=True: a frozen recurrent stack runs in its inference form")
        self.enable_training_objective(state_dict)
        head = "dgrad" if self._face_type == "dgrad_3d" else "offsets"
        optim = self._head_optimizer_args()
        self._head_trainer = HeadTrainer(state_dict, head, device=self._model._engine.device, **optim)
        self._head_trainer_key = register_trainer(self._head_trainer)
        self._head_source = state_dict
        self._attn_trainer = self._attn_trainer_key = None
        self._lstm_trainer = self._lstm_trainer_key = None
        self._lstm0_trainer = self._lstm0_trainer_key = None
        self._freq_trainer = self._freq_trainer_key = None
        self._conv_trainer = self._conv_trainer_key = None
        self._bilstm_dropout = float(bilstm_dropout)
        self._train_flags = dict(attention=bool(attention), bilstm_top=bool(bilstm_top), bilstm_bottom=bool(bilstm_bottom),
                                 bilstm_dropout=float(bilstm_dropout))
        when_set = dict(freq_lstm=freq_lstm, conv_stack=conv_stack)
        assert set(when_set) == set(self._FLAGS_WHEN_SET)
        # the key exists only when set: a state taken without it has the flags it always had
        self._train_flags.update({name: True for name, on in when_set.items() if on})
        if attention:
            from sdfa_amd import attntrain
            # dH is consumed by the BiLSTM layer's backward, and by nothing without it
            self._attn_trainer = attntrain.AttnTrainer(state_dict, device=self._model._engine.device, want_dH=bool(bilstm_top), **optim)
            self._attn_trainer_key = attntrain.register_trainer(self._attn_trainer)
        if bilstm_top:
            from sdfa_amd import lstmtrain
            # dX1 is consumed by the bottom layer's backward, and by nothing while layer 0 is frozen
            self._lstm_trainer = lstmtrain.LstmTrainer(state_dict, layer=1, device=self._model._engine.device, want_dX=bool(bilstm_bottom), **optim)
            self._lstm_trainer_key = lstmtrain.register_trainer(self._lstm_trainer)
        if bilstm_bottom:
            # dX0 is consumed by the frequency LSTM's backward, and by nothing while it is frozen
            self._lstm0_trainer = lstmtrain.LstmTrainer(state_dict, layer=0, device=self._model._engine.device, want_dX=bool(freq_lstm), **optim)
            self._lstm0_trainer_key = lstmtrain.register_trainer(self._lstm0_trainer)
        if freq_lstm:
            from sdfa_amd import freqtrain
            # dC is consumed by the conv stack's backward, and by nothing while it is frozen
            self._freq_trainer = freqtrain.FreqTrainer(state_dict, device=self._model._engine.device, want_dC=bool(conv_stack), **optim)
            self._freq_trainer_key = freqtrain.register_trainer(self._freq_trainer)
        if conv_stack:
            from sdfa_amd import convtrain
            self._conv_trainer = convtrain.ConvTrainer(state_dict, device=self._model._engine.device, **optim)
            self._conv_trainer_key = convtrain.register_trainer(self._conv_trainer)
        return self

    def _bilstm_keep_mask(self, X1):
        """nn.LSTM's inter-layer dropout in training mode: Bernoulli(1 - p) per element of the layer-0 output, over (1 - p)."""
        p = self._bilstm_dropout
        if getattr(self, "_train_generator", None) is None:
            self._train_generator = torch.Generator(device=X1.device)
        keep = torch.empty_like(X1).bernoulli_(1.0 - p, generator=self._train_generator)
        return keep.div_(1.0 - p)

    def _trainer(self):
        tr = getattr(self, "_head_trainer", None)
        if tr is None:
            raise RuntimeError("head training is not enabled: call enable_head_training(state_dict) first")
        return tr

    def train_step(self, batch, i_batch):
        """The reference's train_step (model.py:109-113) for the head: (pred_dict, loss_dict, scalars).  The frozen encoder runs
        through torch.ops.sdfa.encoder without gradient, the head through torch.ops.sdfa.head_train; pred_dict["prediction"]
        holds the coefficients under the key get_loss takes.  sum(loss_dict.values()).backward() leaves the head's gradients
        in the trainer; optimizer_step() is the reference's optim.step().  With enable_head_training(attention=True) the frozen
        stack runs through torch.ops.sdfa.encoder_memory and the attention layer through torch.ops.sdfa.attn_train, which also
        gives align_dict; the backward then leaves the attention layer's gradients in its trainer as well.  With bilstm_top=True
        the frozen stack ends at the layer-0 output (torch.ops.sdfa.encoder_layer0), times the keep mask where bilstm_dropout
        is set, and layer 1 of the BiLSTM runs through torch.ops.sdfa.lstm_train in front of the attention layer.  With
        bilstm_bottom=True the frozen stack ends at the BiLSTM's input (torch.ops.sdfa.encoder_x0) and both layers run through
        torch.ops.sdfa.lstm_train, the keep mask between them inside the graph.  With freq_lstm=True the frozen stack ends at the
        conv stack (torch.ops.sdfa.encoder_conv) and the frequency LSTM runs through torch.ops.sdfa.freq_train in front of them.
        With conv_stack=True the conv stack runs through torch.ops.sdfa.conv_train and no encoder_* operator is called."""
        tr = self._trainer()
        self.train()
        if getattr(self, "_lstm0_trainer", None) is not None:
            # both BiLSTM layers + attention + head: dH flows into layer 1's backward, its dX1 through the keep mask (autograd's
            # product rule: nn.LSTM's inter-layer dropout with both layers trained) into layer 0's; the frequency LSTM and
            # everything below are frozen, so no dX0 is formed
            if getattr(self, "_freq_trainer", None) is not None:
                # the frequency LSTM as well: layer 0's dX0 flows into its backward; while the conv stack is frozen no dC is formed
                if getattr(self, "_conv_trainer", None) is not None:
                    # the conv stack as well: the frequency LSTM's dC flows into its backward; audio_feat is data
                    feat = batch["audio_feat"].contiguous().detach().requires_grad_(True)
                    Cx = torch.ops.sdfa.conv_train(feat, self._conv_trainer_key)
                else:
                    with torch.no_grad():
                        Cx = torch.ops.sdfa.encoder_conv(batch["audio_feat"].contiguous(), self._model._key)
                    Cx = Cx.detach().requires_grad_(True)
                X0 = torch.ops.sdfa.freq_train(Cx, self._freq_trainer_key)
            else:
                with torch.no_grad():
                    X0 = torch.ops.sdfa.encoder_x0(batch["audio_feat"].contiguous(), self._model._key)
                X0 = X0.detach().requires_grad_(True)
            X1 = torch.ops.sdfa.lstm_train(X0, self._lstm0_trainer_key)
            if self._bilstm_dropout > 0.0:
                with torch.no_grad():
                    keep = self._bilstm_keep_mask(X1)
                X1 = X1 * keep
            H = torch.ops.sdfa.lstm_train(X1, self._lstm_trainer_key)
            z, align = torch.ops.sdfa.attn_train(H, self._attn_trainer_key)
            align = align.detach()
        elif getattr(self, "_lstm_trainer", None) is not None:
            # BiLSTM top layer + attention + head: dz flows from the head's backward into the attention layer's, its dH into the
            # BiLSTM layer's; layer 0 and everything below are frozen, so no dX1 is formed
            with torch.no_grad():
                X1 = torch.ops.sdfa.encoder_layer0(batch["audio_feat"].contiguous(), self._model._key)
                if self._bilstm_dropout > 0.0:
                    X1 = X1 * self._bilstm_keep_mask(X1)
            X1 = X1.detach().requires_grad_(True)
            H = torch.ops.sdfa.lstm_train(X1, self._lstm_trainer_key)
            z, align = torch.ops.sdfa.attn_train(H, self._attn_trainer_key)
            align = align.detach()
        elif getattr(self, "_attn_trainer", None) is not None:
            # attention + head: the frozen stack up to the BiLSTM output H, then the two trained stages; dz flows from the head's
            # backward into the attention layer's, whose parameter gradients stay in its trainer
            with torch.no_grad():
                H, _, _ = torch.ops.sdfa.encoder_memory(batch["audio_feat"].contiguous(), self._model._key)
            H = H.detach().requires_grad_(True)
            z, align = torch.ops.sdfa.attn_train(H, self._attn_trainer_key)
            align = align.detach()
        else:
            with torch.no_grad():
                z, align = torch.ops.sdfa.encoder(batch["audio_feat"].contiguous(), self._model._key)
            z = z.detach().requires_grad_(True)      # the head's parameters live in the trainer: the graph hangs on z, whose gradient is dz
        coef = torch.ops.sdfa.head_train(z, batch["speaker_id"], self._head_trainer_key)
        name = "dgrad_3d_coef" if self._face_type == "dgrad_3d" else f"{self._face_type}_coef"
        pred_dict = dict(prediction={name: coef}, condition=z.view(-1, 1, 512), align_dict={"audio_encoder10": align.view(-1, 1, 64)}, latent_dict={})
        loss_dict, scalars = self.get_loss(pred_dict, batch)
        assert tr.coef_dim == coef.shape[1]
        return pred_dict, loss_dict, scalars

    def optimizer_step(self):
        tr, at, lt = self._trainer(), getattr(self, "_attn_trainer", None), getattr(self, "_lstm_trainer", None)
        l0 = getattr(self, "_lstm0_trainer", None)
        if at is not None and at.step_count != tr.step_count:
            raise RuntimeError(f"head trainer at step {tr.step_count}, attention trainer at step {at.step_count}: they step together")
        if lt is not None and lt.step_count != tr.step_count:
            raise RuntimeError(f"head trainer at step {tr.step_count}, BiLSTM trainer at step {lt.step_count}: they step together")
        if l0 is not None and l0.step_count != tr.step_count:
            raise RuntimeError(f"head trainer at step {tr.step_count}, BiLSTM bottom-layer trainer at step {l0.step_count}: they step together")
        fq = getattr(self, "_freq_trainer", None)
        if fq is not None and fq.step_count != tr.step_count:
            raise RuntimeError(f"head trainer at step {tr.step_count}, frequency-LSTM trainer at step {fq.step_count}: they step together")
        cv = getattr(self, "_conv_trainer", None)
        if cv is not None and cv.step_count != tr.step_count:
            raise RuntimeError(f"head trainer at step {tr.step_count}, conv-stack trainer at step {cv.step_count}: they step together")
        tr.step()
        if at is not None:
            at.step()
        if lt is not None:
            lt.step()
        if l0 is not None:
            l0.step()
        if fq is not None:
            fq.step()
        if cv is not None:
            cv.step()

    def fit_head(self, trainset, steps, rng, batch_size=50, noise="device", fixed_batch=None):
        """`steps` steps of the reference's loop (trainer.py:266-320: train_step, the summed losses' backward, optim.step) over
        DatasetSlidingWindow.train_batch on `trainset` (a TrainSet); rng: numpy RandomState for the indices and the augmentation.
        fixed_batch: train on this one batch instead.  Returns the scalars of every step."""
        history = []
        for i in range(int(steps)):
            if fixed_batch is not None:
                batch = fixed_batch
            else:
                idx = rng.randint(0, len(trainset), int(batch_size))
                batch = DatasetSlidingWindow.train_batch(trainset, None, idx, rng, noise=noise, hparams=self.hp)
            _, loss_dict, scalars = self.train_step(batch, i)
            sum(loss_dict.values()).backward()
            self.optimizer_step()
            history.append(scalars)
        return history

    def head_state_dict(self):
        """The tuned head under the reference's names ("_model._output_module. ... weight_g | weight_v | bias"), and with
        attention training enabled the tuned attention tensors ("_model._audio_encoder._layers.10. ..."), with bilstm_top the
        four tuned layer-1 tensors of the BiLSTM ("_model._audio_encoder._layers.9.weight_ih_l1 ..."), with bilstm_bottom the
        four layer-0 tensors ("... weight_ih_l0", "weight_hh_l0" and their "_reverse" twins), with freq_lstm the ten tensors of
        the frequency LSTM and its projection ("_model._audio_encoder._layers.6._lstm. ...", "..._proj.weight | bias"), with
        conv_stack the 15 tensors of the conv stack ("_model._audio_encoder._layers.1 | 3 | 5.weight_g | weight_v | bias |
        _ext_post_bn.weight | _ext_post_bn.bias"; the running statistics are not trained)."""
        tuned = self._trainer().head_state_dict()
        if getattr(self, "_attn_trainer", None) is not None:
            tuned.update(self._attn_trainer.attn_state_dict())
        if getattr(self, "_lstm_trainer", None) is not None:
            tuned.update(self._lstm_trainer.lstm_state_dict())
        if getattr(self, "_lstm0_trainer", None) is not None:
            tuned.update(self._lstm0_trainer.lstm_state_dict())
        if getattr(self, "_freq_trainer", None) is not None:
            tuned.update(self._freq_trainer.freq_state_dict())
        if getattr(self, "_conv_trainer", None) is not None:
            tuned.update(self._conv_trainer.conv_state_dict())
        return tuned

    # ---- save, stop, resume: what a training loop around train_step has to carry ----
    _TRAINER_SLOTS = (("head", "_head_trainer"), ("attention", "_attn_trainer"), ("bilstm_top", "_lstm_trainer"), ("bilstm_bottom", "_lstm0_trainer"),
                      ("freq_lstm", "_freq_trainer"), ("conv_stack", "_conv_trainer"))
    _FLAGS_WHEN_SET = ("freq_lstm", "conv_stack")       # flags whose key exists only when true

    def training_state_dict(self):
        """Everything a fit needs to continue bit for bit: every enabled trainer's state_dict() (parameters, both Adam moments,
        the step count, the optimiser arguments) under "head", "attention", "bilstm_top", "bilstm_bottom", "freq_lstm", "conv_stack"; the
        DynamicLossScalers' state by the reference's names; the dropout generator's state (None while nothing has been drawn);
        and the flags enable_head_training was called with.  Host data only, so torch.save takes it."""
        self._trainer()
        trainers = {name: getattr(self, attr).state_dict() for name, attr in self._TRAINER_SLOTS if getattr(self, attr, None) is not None}
        gen = getattr(self, "_train_generator", None)
        return dict(flags=dict(self._train_flags), trainers=trainers,
                    scalers={name: sc.state_dict() for name, sc in self._loss_scalers.items()},
                    generator=None if gen is None else gen.get_state().clone())

    def load_training_state_dict(self, state):
        """Continue from training_state_dict() on a model enabled with the same flags; a state taken with other flags is refused
        by name, before anything is changed."""
        self._trainer()
        theirs, mine = dict(state["flags"]), self._train_flags
        differ = [f"{k}={theirs.get(k)!r} (this model: {k}={mine[k]!r})" for k in mine if k not in self._FLAGS_WHEN_SET and theirs.get(k) != mine[k]]
        for k in self._FLAGS_WHEN_SET:                  # a key that exists only when set: absent is False, either way round
            a, b = bool(theirs.get(k, False)), bool(mine.get(k, False))
            if a != b:
                differ.append(f"{k}={a!r} (this model: {k}={b!r})")
        if differ or set(theirs) != set(mine):
            raise ValueError("training state: taken with " + ", ".join(differ or sorted(set(theirs) ^ set(mine))) +
                             ": enable_head_training must be called with the flags the state was taken with")
        enabled = {name for name, attr in self._TRAINER_SLOTS if getattr(self, attr, None) is not None}
        if set(state["trainers"]) != enabled:
            raise ValueError(f"training state: holds the trainers {sorted(state['trainers'])}, this model has {sorted(enabled)}")
        for name, attr in self._TRAINER_SLOTS:
            if name in enabled:
                getattr(self, attr).load_state_dict(state["trainers"][name])
        self._loss_scalers = dict()
        for name, sc in state["scalers"].items():
            self._scaler(name).load_state_dict(sc)
        if state.get("generator") is None:
            self._train_generator = None
        else:
            self._train_generator = torch.Generator(device=self._model._engine.device)
            self._train_generator.set_state(state["generator"])
        return self

    def commit_head(self):
        """A fresh inference engine from the original state dict with the tuned head in it, through the same weights.py route
        as load_state_dict (the weight norm folded, strict shapes); generate_animation uses it from here on.  The trainer and
        its Adam state stay as they are."""
        tuned = self.head_state_dict()
        src = self._head_source
        prefixed = any(k.startswith("_model.") for k in src)
        state = dict(src)
        for k, v in tuned.items():
            key = k if prefixed else k[len("_model."):]
            assert key in state, key
            state[key] = v
        self.load_state_dict(state)
        self.enable_training_objective(state)
        return self

    # ---- model.py:333-420 ---------------------------------------------------------------------
    @staticmethod
    def _check_signal(signal):
        """The input checks of generate_animation (model.py:339-349)."""
        if torch.is_tensor(signal):
            if signal.dim() > 1:
                assert signal.dim() == 2
                assert signal.size(0) == 1
                signal = signal[0]
            signal = signal.detach().cpu().numpy()
        assert isinstance(signal, np.ndarray)
        assert np.prod(signal.shape) == np.max(signal.shape)
        assert signal.min() >= -1
        assert signal.max() <= 1
        return np.asarray(signal.flatten(), np.float32)

    @torch.no_grad()
    def generate_animation(self, signal, speaker, emotion, frame_id, ensembling_ms=None, dataset_class=None, **kwargs):
        """(tslist, animes (F, 9976, 9) | (F, 15069) float32 numpy, others) for ONE clip -- the reference's signature and result.

        The default dataset class takes the device pipeline of `generate_animation_batch` (one front-end call, column-sharing
        encoder, ensembling mean on the device, one pinned device -> host copy); a caller-supplied `dataset_class` keeps the
        reference's two-step route through its `fetch_audio_features` and `_feature_to_anime`.  `animes` is a view of pinned host
        memory owned by the returned array.  kwargs: want_inputs (default True, as the reference returns others["inputs"]);
        filter_anime (default None): a sdfa_amd.tfilter.parse_filter spec, "gaussian:SIGMA" or
        "bilateral:DISTANCE_SIGMA,RANGE_SIGMA,RADIUS[,FACTOR]" -- the rows are filtered along time on the device where the
        reference's identity hook _filter_anime sits (model.py:405-406,420), after the ensembling mean."""
        signal = self._check_signal(signal)
        filter_anime = kwargs.get("filter_anime")
        if filter_anime is not None:
            from sdfa_amd.tfilter import parse_filter
            filter_anime = parse_filter(filter_anime)                   # a bad spec is refused before any device work
        if dataset_class is None:
            dataset_class = DatasetSlidingWindow
        if isinstance(speaker, str):
            speaker = self._speakers_dict[speaker]
        if isinstance(emotion, str):
            emotion = self._emotions_dict[emotion]
        if ensembling_ms is None:
            ensembling_ms = self.hp.ensembling_ms
        if dataset_class is DatasetSlidingWindow:
            return self._animate([signal], [speaker], ensembling_ms, kwargs.get("want_inputs", True), filter_anime)[0]

        passes = [signal]
        if ensembling_ms is not None and ensembling_ms > 0:            # model.py:373-384: second pass on a delayed copy
            pad = ensembling_ms * self.hp.audio.sample_rate // 1000
            passes.append(np.pad(signal[:-pad], [[pad, 0]], "constant"))
        feats = [dataset_class.fetch_audio_features(p, self.hp) for p in passes]
        anime_sum, others = self._feature_to_anime(feats[0]["audio_feat"], feats[0]["energy"], speaker, emotion, frame_id,
                                                   want_inputs=kwargs.get("want_inputs", True))
        for f in feats[1:]:
            anime_sum += self._feature_to_anime(f["audio_feat"], f["energy"], speaker, emotion, frame_id, want_inputs=False)[0]
        if len(feats) > 1:
            anime_sum = anime_sum / float(len(feats))
        if filter_anime is not None:
            flat = torch.from_numpy(np.ascontiguousarray(anime_sum, np.float32)).reshape(len(anime_sum), -1)
            anime_sum = self._filter_rows(flat, [len(flat)], filter_anime).numpy().reshape(anime_sum.shape)
        return feats[0]["tslist"], anime_sum, others

    @torch.no_grad()
    def generate_animation_batch(self, signals, speakers, emotions=0, frame_id=0, ensembling_ms=None, want_inputs=False, filter_anime=None):
        """Several utterances through ONE launch group: [(tslist, animes, others)] in the order of `signals`, each exactly
        what `generate_animation` returns for that clip alone (frames are independent and a column's features do not depend
        on the batch, so the rows are bitwise the single-clip rows).  `speakers`: one name / id, or one per clip.
        `filter_anime`: as in generate_animation; every clip is filtered on its own, never across a clip boundary."""
        signals = [self._check_signal(s) for s in signals]
        if filter_anime is not None:
            from sdfa_amd.tfilter import parse_filter
            filter_anime = parse_filter(filter_anime)
        if isinstance(speakers, (str, int, np.integer)):
            speakers = [speakers] * len(signals)
        assert len(speakers) == len(signals)
        speakers = [self._speakers_dict[s] if isinstance(s, str) else s for s in speakers]
        if ensembling_ms is None:
            ensembling_ms = self.hp.ensembling_ms
        return self._animate(signals, speakers, ensembling_ms, want_inputs, filter_anime)

    def animation_stream(self, speaker, emotion=0, frame_id=0, ensembling_ms=None, input_rate=None, gain=1.0):
        """generate_animation for audio that arrives in pieces: an object whose push(chunk) and finish() each return
        (tslist, animes) shaped like generate_animation's; concatenated, they are generate_animation(signal, ...)[:2] of the
        whole signal, bit for bit.  Frames are returned as soon as their window has arrived (sdfa_amd.live.LiveSession).
        With `input_rate` the chunks are at that rate and are converted on the device: the result is that of the signal
        clip(sdfa_amd.resample.resample(x, input_rate, sample_rate) * float32(gain), -0.999, 0.999)."""
        eng = self._model._engine
        if eng is None:
            raise RuntimeError("no weights loaded: call load_state_dict first")
        if isinstance(speaker, str):
            speaker = self._speakers_dict[speaker]
        assert isinstance(speaker, (int, np.integer)), f"given index is {speaker}, {type(speaker)}"
        if ensembling_ms is None:
            ensembling_ms = self.hp.ensembling_ms
        return AnimationStream(self, int(speaker), int(ensembling_ms or 0), input_rate, gain)

    def _filter_rows(self, rows, counts, spec, device_rows=None):
        """The filter_anime hook: the pinned host rows of consecutive clips (`counts` frames each) are filtered along time on the
        device, clip by clip, and written back in place.  `device_rows`: their device copy when it is still there, else they are
        uploaded.  evaluate (self._keep_filtered) also keeps the filtered device rows, for its exports.  Returns rows."""
        from sdfa_amd import tfilter
        eng = self._model._engine
        n = int(sum(counts))
        off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        src = device_rows if device_rows is not None else rows[:n].to(eng.device)
        filtered = tfilter.apply(spec, src.reshape(n, -1), clip_frame_off=off)
        rows[:n].copy_(filtered)
        self._filtered_rows = filtered if getattr(self, "_keep_filtered", False) else None
        return rows

    def _animate(self, signals, speakers, ensembling_ms, want_inputs, filter_anime=None):
        from sdfa_amd.engine import frame_index
        eng = self._model._engine
        if eng is None:
            raise RuntimeError("no weights loaded: call load_state_dict first")
        sr = self.hp.audio.sample_rate
        for spk in speakers:
            assert isinstance(spk, (int, np.integer)), f"given index is {spk}, {type(spk)}"
            eng.check_speaker_ids(int(spk))
        ensemble = ensembling_ms is not None and ensembling_ms > 0
        # The reference keeps the features of the LAST signal (model.py:364-367,409-416): the same audio with another speaker does
        # not recompute the front end.  Here everything up to the encoder output z is speaker-independent, so the one-entry cache
        # holds z: a speaker sweep over one clip re-runs only the regressor (bitwise the full call: same z, same kernels after it).
        # The key carries everything that changes z for a given signal: rate, ensembling delay, precision mode and the library's
        # option epoch (sdfa_amd._lib.set_option; a switch set through the raw C call needs clear_signal_cache()).
        # hparams.signal_cache = False turns the cache off (it pins z and up to 256 MB of features on the device).
        from sdfa_amd import _lib as _sdfa_lib
        use_cache = bool(self.hp.get("signal_cache", True))
        key = (sr, int(ensembling_ms) if ensemble else 0, eng.precision, _sdfa_lib.option_epoch)
        c = getattr(self, "_signal_cache", None) if use_cache else None
        if (len(signals) == 1 and c is not None and c["key"] == key and c["signal"].shape == signals[0].shape
                and (c["feat"] is not None or not want_inputs) and np.array_equal(c["signal"], signals[0])):
            n = len(c["tslist"])
            spk = torch.full((n,), int(speakers[0]), dtype=torch.int64, device=eng.device)
            inputs_host = eng.to_host_async(c["feat"][:n].permute(0, 3, 2, 1)) if want_inputs else None
            rows = eng.forward_host(None, spk, z=c["z"], ops_key=self._model._key, wait=True, ensemble=ensemble)
            if filter_anime is not None:
                self._filter_rows(rows, [n], filter_anime, eng.last_device_rows(n))
            return [self._pack(rows.numpy(), None if inputs_host is None else inputs_host.numpy(), [list(c["tslist"])], [n])[0]]
        self._signal_cache = None
        tables = [frame_index(len(s), sr) for s in signals]             # ONE enumeration per clip (starts, tslist)
        clips = list(signals)
        if ensemble:                                                    # model.py:373-384: second pass on a delayed copy --
            pad = ensembling_ms * sr // 1000                            # here as further clips of the same launch group
            clips += [np.pad(s[:-pad], [[pad, 0]], "constant") for s in signals]
            tables = tables + tables
        feat, tslists, counts = eng.mel_frontend(clips, sr, tables=tables)
        share = eng.last_frame_table                                    # (clip, start, hop): the per-column stages run once per distinct column
        tslists, counts = tslists[:len(signals)], counts[:len(signals)]
        n = int(sum(counts))
        spk = torch.from_numpy(np.repeat(np.asarray(speakers, np.int64), counts)).to(eng.device, non_blocking=True)
        inputs_host = None
        if want_inputs:                                                 # others["inputs"] = audio_feat.permute(0, 3, 2, 1), model.py:463-466
            inputs_host = eng.to_host_async(feat[:n].permute(0, 3, 2, 1))
        rows = eng.forward_host(feat, spk, table=share, ops_key=self._model._key, wait=True, ensemble=ensemble)
        if use_cache and len(signals) == 1 and eng.last_z() is not None:   # one clip, one piece: remember (signal -> z) for a speaker sweep
            # z is 2 KB per frame; the features (others["inputs"] of a later hit) are 98 KB per frame and are kept up to 256 MB only
            keep_feat = feat if feat.numel() * 4 <= (256 << 20) else None
            self._signal_cache = {"key": key, "signal": signals[0].copy(), "tslist": list(tslists[0]), "z": eng.last_z(), "feat": keep_feat}
        if filter_anime is not None:
            self._filter_rows(rows, counts, filter_anime, eng.last_device_rows(n))
        return self._pack(rows.numpy(), inputs_host.numpy() if inputs_host is not None else None, tslists, counts)

    def _pack(self, rows_np, inputs_np, tslists, counts):
        shape = (-1, 9) if self._face_type == "dgrad_3d" else ()
        out, f0 = [], 0
        for ci, c in enumerate(counts):
            animes = rows_np[f0:f0 + c].reshape((c,) + shape) if shape else rows_np[f0:f0 + c]
            others = {"inputs": inputs_np[f0:f0 + c] if inputs_np is not None else None,
                      "phones": None, "latent": None, "latent_align": None, "formants": None}
            out.append((tslists[ci], animes, others))
            f0 += c
        return out

    # ---- model.py:428-489 ---------------------------------------------------------------------
    @torch.no_grad()
    def _feature_to_anime(self, feat_list, energy_list, speaker_id, emotion_id, frame_id, bs=100, want_inputs=True):
        """audio_feat (F,64,128,3) (numpy or tensor, any device) -> (animes (F, 9976, 9) | (F, 15069) float32 numpy, others).
        `bs` is accepted for signature parity; frames are independent, so the engine batches by its own chunk size and the rows
        reach the host through pinned memory while the next piece computes (Engine.forward_host)."""
        assert isinstance(speaker_id, (int, np.integer)), f"given index is {speaker_id}, {type(speaker_id)}"
        eng = self._model._engine
        eng.check_speaker_ids(int(speaker_id))      # before any device work: ids >= num_speakers raise like one_hot's scatter_
        feat = feat_list if torch.is_tensor(feat_list) else torch.from_numpy(np.asarray(feat_list, np.float32))
        feat = feat.to(eng.device, dtype=torch.float32).contiguous()
        n = feat.shape[0]
        inputs_host = eng.to_host_async(feat.permute(0, 3, 2, 1)) if want_inputs else None
        rows = eng.forward_host(feat, int(speaker_id), ops_key=self._model._key, wait=True)
        animes = rows.numpy()
        if self._face_type == "dgrad_3d":
            animes = animes.reshape(n, -1, 9)
        others = {"inputs": inputs_host.numpy() if inputs_host is not None else None,
                  "phones": None, "latent": None, "latent_align": None, "formants": None}
        return animes, others

    # ---- model.py:261-330 (get_loss's scalars on held-out tracks) ---------------------------------
    @torch.no_grad()
    def validate(self, clips, frames="inference", anime_loss_weight=None, keep_rows=False):
        """The reference's validation scalars (get_loss with PLoss / MLoss, criterion.py) of this checkpoint on held-out clips:
        {"clips": [per clip: scalar_ps, scalar_pr, scalar_ms, scalar_mr, scalar_ploss, scalar_mloss, frames], "corpus": the same keys,
        the mean over clips weighted by their frame counts}.  The offsets head carries its whole loss in scalar_ps / scalar_ms
        (= scalar_ploss / scalar_mloss; pr = mr = 0).

        clips: each (signal, speaker, track, start_ts, anime_minfi, anime_maxfi) or a dict with those keys (`minfi`, `maxfi`;
        optionally `lips_dist`): track = the float32 rows of track frames anime_minfi .. anime_maxfi, or a directory of NNNNNN.npy.
        frames: "inference" scores the frames generate_animation produces (sdfa_frame_index); "dataset" the windows the
        reference's dataset enumerates (sliding_window.py:45-61), without its random shift.  One pass, no ensembling, as the
        reference validates.  anime_loss_weight="anime_weight" weights the frames by exp((0.002 - lips_dist) * 50) * 2.
        The rows stay on the device; sdfa_amd.score reads each prediction element once.
        Absent: ELoss (no evector here) and DynamicLossScaler (its state is not in a checkpoint)."""
        from sdfa_amd import score
        from sdfa_amd.engine import frame_index, frame_geometry
        from .. import validate as _v
        eng = self._model._engine
        if eng is None:
            raise RuntimeError("no weights loaded: call load_state_dict first")
        if frames not in ("inference", "dataset"):
            raise ValueError(f"frames must be 'inference' or 'dataset', got {frames!r}")
        if anime_loss_weight not in (None, "anime_weight"):
            raise ValueError(f"anime_loss_weight must be None or 'anime_weight', got {anime_loss_weight!r}")
        sr, fps, ts_delta = self.hp.audio.sample_rate, self.hp.anime.fps, self.hp.anime.feature.ts_delta
        sliding = frame_geometry(sr)[2]
        signals, speakers, tables, tracks, plans, weights, base = [], [], [], [], [], [], 0
        for ci, clip in enumerate(clips):
            c = clip if isinstance(clip, dict) else dict(zip(("signal", "speaker", "track", "start_ts", "minfi", "maxfi"), clip))
            signal = self._check_signal(c["signal"])
            spk = self._speakers_dict[c["speaker"]] if isinstance(c["speaker"], str) else c["speaker"]
            eng.check_speaker_ids(int(spk))
            minfi, maxfi = int(c["minfi"]), int(c["maxfi"])
            track = _v.load_track(c["track"], minfi, maxfi) if isinstance(c["track"], (str, os.PathLike)) else c["track"]
            track = (track if torch.is_tensor(track) else torch.from_numpy(np.asarray(track, np.float32))).reshape(maxfi - minfi + 1, -1)
            if frames == "inference":
                starts, ts = frame_index(len(signal), sr, fps, ts_delta)
            else:
                starts = score.dataset_frame_starts(len(signal), sr, fps, sliding)
                ts = np.zeros(len(starts), np.int32)
            if len(starts) < 2:
                raise ValueError(f"clip {ci}: {len(starts)} frame, the motion loss needs at least 2")
            src, w = score.truth_plan(starts, sr, float(c["start_ts"]), minfi, maxfi, fps, ts_delta, sliding)
            if anime_loss_weight is not None:
                if c.get("lips_dist") is None:
                    raise ValueError(f"clip {ci}: anime_loss_weight needs the track's lips_dist values")
                weights.append(score.anime_weights(c["lips_dist"], src - minfi, w))
            plans.append((src - minfi + base, w))
            base += track.shape[0]
            signals.append(signal); speakers.append(int(spk)); tables.append((starts, ts)); tracks.append(track)
        feat, _, counts = eng.mel_frontend(signals, sr, tables=tables)
        fclip, fstart, hop = eng.last_frame_table
        n = int(sum(counts))
        spk = torch.from_numpy(np.repeat(np.asarray(speakers, np.int64), counts)).to(eng.device)
        rows = torch.empty((n, eng.out_dim), dtype=torch.float32, device=eng.device)
        for f0 in range(0, n, eng.max_frames):                           # the batch path's launch groups; the rows never leave the device
            f1 = min(n, f0 + eng.max_frames)
            z, _ = eng.encoder(feat[f0:f1], want_align=False, frame_clip=fclip[f0:f1], frame_start=fstart[f0:f1], hop=hop)
            eng.regress(z, spk[f0:f1], out=rows[f0:f1], check_ids=False)
        d_track = torch.cat([t.to(device=eng.device, dtype=torch.float32) for t in tracks])
        assert d_track.shape[1] == eng.out_dim, f"track rows of {d_track.shape[1]} values, the head writes {eng.out_dim}"
        off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        dgrad = self._face_type == "dgrad_3d"
        rec = score.score_rows(rows, d_track, np.concatenate([p[0] for p in plans]), np.concatenate([p[1] for p in plans]), off,
                               score.LAYOUT_DGRAD if dgrad else score.LAYOUT_PLAIN)
        res = score.clip_scalars(rec, off, eng.out_dim // 9 if dgrad else eng.out_dim, np.concatenate(weights) if weights else None)
        if keep_rows:
            res.update(rows=rows, records=rec, plan=(np.concatenate([p[0] for p in plans]), np.concatenate([p[1] for p in plans])), track=d_track,
                       clip_frame_off=off)
        return res

    # ---- model.py:121-223 (host loop: dgrad track dump, mesh export, video rendered on the GPU) ----
    def evaluate(self, sources, experiment=None, in_trainer=False, **kwargs):
        """The reference's host loop over sources (model.py:152-212).  The reference calls generate_animation once per source; here
        the sources are taken in LAUNCH GROUPS -- as many consecutive clips as fit one piece of the engine (`max_frames` animation
        frames; kwargs["group_frames"] overrides) go through ONE generate_animation_batch call -- because frames are independent
        and a clip's rows do not depend on what it is batched with (bitwise, tests/test_surface_fast.py), so every per-clip result
        and every file written is exactly what the clip-by-clip loop produces, at the batch path's throughput.

        kwargs["save_video"] (the reference's --save_video): also write <output_dir>/<name>.avi, grid_w x grid_h, rendered on the GPU
        from the template mesh (speech_anime.video); it needs a template (--template_mesh) and fails before any device work without
        one.  Titles and the truth / latent / alignment panels of the reference's grid are not drawn.  kwargs["jpeg_encoder"]: "pil"
        (default, host threads) or "gpu" (sdfa_amd.jpeg) encodes the video's frames; both write the same bytes.
        kwargs["filter_anime"]: a temporal filter spec as in generate_animation; everything returned, written, exported or rendered
        is the filtered track."""
        filter_anime = kwargs.get("filter_anime")
        if filter_anime is not None:
            from sdfa_amd.tfilter import parse_filter
            filter_anime = parse_filter(filter_anime)
        save_video = bool(kwargs.get("save_video", False))
        jpeg_encoder = kwargs.get("jpeg_encoder") or "pil"
        from .. import video as _video
        if jpeg_encoder not in _video.JPEG_ENCODERS:
            raise ValueError(f"jpeg_encoder must be one of {_video.JPEG_ENCODERS}, not {jpeg_encoder!r}")
        if kwargs.get("source_mesh") is not None:       # not a reference kwarg: retarget the offsets head (viewer.set_source_mesh)
            from .. import viewer
            viewer.set_source_mesh(kwargs["source_mesh"])
        if save_video:
            from .. import viewer
            if not viewer.has_template():
                raise ValueError("save_video needs a template mesh (--template_mesh <obj>): the video is rendered from it.  The reference "
                                 "falls back to its bundled FLAME_sample.obj, which is not part of this tree")
            skipped = [k for k in ("with_title", "draw_truth", "draw_align", "draw_latent") if kwargs.get(k)]
            if skipped:
                print(f"[speech_anime] evaluate: {', '.join(skipped)} not supported: the video shows the inferred face only, without title")
        video_size = (int(kwargs.get("grid_w") or 512), int(kwargs.get("grid_h") or 512))
        sr = self.hp.audio.sample_rate
        output_dir = kwargs.get("output_dir") or "evaluate_results"
        target_db = kwargs.get("audio_target_db", self.hp.dataset_anime.audio_target_db)
        export_frames = kwargs.get("export_mesh_frames", not in_trainer)
        ens = kwargs.get("ensembling_ms")
        if ens is None:
            ens = self.hp.ensembling_ms
        eng = self._model._engine
        if eng is None:
            raise RuntimeError("no weights loaded: call load_state_dict first")
        from sdfa_amd.engine import frame_index
        limit = int(kwargs.get("group_frames") or eng.max_frames) // (2 if (ens is not None and ens > 0) else 1)
        # the reference's evaluate returns nothing; the mirror returns [(path, tslist, animes)] for callers that want the tracks (the
        # rows are views of pinned host memory: a long evaluation that only wants the files passes keep_results=False, as the CLI does)
        keep = bool(kwargs.get("keep_results", True))
        results, group, group_frames = [], [], 0

        def flush():
            nonlocal group, group_frames
            if not group:
                return
            if filter_anime is not None:
                self._keep_filtered = export_frames or save_video
            outs = self.generate_animation_batch([g["signal"] for g in group], [g["spk"] for g in group], ensembling_ms=ens, want_inputs=False,
                                                 filter_anime=filter_anime)
            total = sum(len(o[0]) for o in outs)
            track_all = eng.last_device_rows(total) if (export_frames or save_video) else None      # one piece: the rows are still on the device
            if filter_anime is not None and track_all is not None:
                track_all = self._filtered_rows                        # the staging buffer holds the unfiltered rows
            f0 = 0
            for g, (tslist, animes, _) in zip(group, outs):
                track = None if track_all is None else track_all[f0:f0 + len(tslist)]
                f0 += len(tslist)
                self._write_result(g, tslist, animes, track, output_dir, export_frames, video_size if save_video else None,
                                   jpeg_encoder)
                if keep:
                    results.append((g["path"], tslist, animes))
            if filter_anime is not None:
                self._keep_filtered, self._filtered_rows = False, None
            group, group_frames = [], 0

        # Utterance-level shards (north_star): with kwargs["shard"] = (rank, world) rank r takes a contiguous block of the
        # flat source list -- sizes differ by at most one -- and writes its own sources' files; frames are independent, so no exchange
        # is needed and every file is what the single-process run writes.  WITHOUT `shard` every source is processed, as the reference's
        # evaluate does (model.py:152-212), whatever RANK / WORLD_SIZE say: only the process entry point (`speech_anime.api.evaluate_model`,
        # i.e. `python -m torch.distributed.run ... -m speech_anime evaluate`) derives the shard from the environment and passes it down.
        flat = [rec for _, records in dict(sources).items() for rec in records]
        rank, world = kwargs.get("shard") or (0, 1)
        if world > 1:
            from sdfa_amd.dist import shard_range
            lo, hi = shard_range(len(flat), rank, world)
            print(f"[speech_anime] evaluate: shard {rank} of {world} takes sources [{lo}, {hi}) of {len(flat)} ({len(flat) - (hi - lo)} left to the other ranks)")
            flat = flat[lo:hi]
        for records in (flat,):
            for rec in records:
                path = rec[0]
                spk = "m1"
                for extra in rec[1:]:
                    if isinstance(extra, str) and extra.startswith("speaker="):
                        spk = extra.split("=", 1)[1]
                signal, sound_signal = _audio.load_source(path, sr, return_sound=True)         # eval_utils.py:76-86
                signal = _audio.rms_normalize(signal, target_db).astype(np.float32)            # model.py:165
                signal = self._check_signal(signal)
                n = int(frame_index(len(signal), sr)[0].shape[0])
                if group and group_frames + n > limit:
                    flush()
                group.append(dict(path=path, spk=spk, signal=signal, sound=sound_signal))
                group_frames += n
        flush()
        return results

    def _write_result(self, g, tslist, animes, track, output_dir, export_frames, video_size=None, jpeg_encoder="pil"):
        """One source's files (model.py:195-223): tslist / track dumps, audio.wav, NNNNNN_dgrad.npy and, with a template, NNNNNN.obj;
        with `video_size` = (grid_w, grid_h) also <output_dir>/<name>.avi (viewer.render_video, model.py:214-223)."""
        fps = self.hp.anime.fps
        name = os.path.splitext(os.path.basename(g["path"]))[0]
        out_dir = os.path.join(output_dir, name)
        os.makedirs(out_dir, exist_ok=True)
        np.save(os.path.join(out_dir, "tslist.npy"), np.asarray(tslist, np.int64))
        np.save(os.path.join(out_dir, f"{self._face_type}.npy"), animes)
        if export_frames:                                                              # model.py:201-212
            from .. import viewer
            from sdfa_amd.seek import SeekPlan
            eng = self._model._engine
            if g["sound"] is not None:
                _audio.write_wav(os.path.join(out_dir, "audio.wav"), g["sound"], _audio.SOUND_SR)   # model.py:203
            # stream.seek for every video frame i at i * 1000 / fps, i = 0 .. int(tslist[-1] * fps / 1000), as ONE
            # device stage; with a template the mesh solve is fused into it (the blended track is only
            # materialised for the NNNNNN_dgrad.npy dump the reference also writes)
            plan = SeekPlan([tslist], fps, device=eng.device)
            if track is None:                                       # the group took several pieces: re-upload this clip's rows (model.py:200)
                track = torch.from_numpy(np.ascontiguousarray(animes, dtype=np.float32)).to(eng.device).reshape(len(tslist), -1)
            rows = plan.rows(track)
            frames = rows.cpu().numpy().reshape((plan.n_queries,) + animes.shape[1:])
            for i_frame, data_frame in enumerate(frames):
                np.save(os.path.join(out_dir, f"{i_frame:06d}_dgrad.npy"), data_frame)
            if viewer.has_template():          # --template_mesh given: seek + solve on the GPU, then .obj per frame, its text
                if self._face_type == "dgrad_3d":                                       # formatted there too (sdfa_amd.obj)
                    verts = viewer.track_to_mesh(track, plan)
                else:     # offsets head: with a source mesh retargeted on the device (deform_grad + the template's solve), else + template
                    verts = viewer._device_verts(rows, self._face_type)
                viewer.write_obj_frames(out_dir, verts, viewer.template_faces())
        if video_size is not None:
            video_path = os.path.join(output_dir, name + ".avi")        # model.py:197-203: export_dir = splitext(video_path)[0]
            self._write_video(video_path, g, tslist, animes, track, video_size, jpeg_encoder)
            print(f"[speech_anime] {name}: {len(tslist)} animation frames -> {out_dir}, {video_path}")
        else:
            print(f"[speech_anime] {name}: {len(tslist)} animation frames -> {out_dir}")

    def _write_video(self, video_path, g, tslist, animes, track, video_size, jpeg_encoder="pil"):
        """viewer.render_video for the inferred source alone (video.py:199-290): frame k is video frame k of the seek plan,
        seek + solve + render on the GPU, encoded to MJPEG on host threads (jpeg_encoder="pil", after a readback in chunks) or
        on the GPU ("gpu", only the JPEG files are read back), with the 44.1 kHz sound.

        The frame COUNT is the reference's loop (ts accumulated in float64, speech_anime.video.video_frame_count); frame k is
        blended at k * 1000 / fps like the .obj export (the accumulated ts differs from it by ~1e-12 ms)."""
        from .. import viewer, video
        from sdfa_amd.seek import SeekPlan
        eng = self._model._engine
        fps = self.hp.anime.fps
        plan = SeekPlan([tslist], fps, device=eng.device)
        n = video.video_frame_count(tslist[-1], fps)
        assert n <= plan.n_queries, (n, plan.n_queries)
        if track is None:
            track = torch.from_numpy(np.ascontiguousarray(animes, dtype=np.float32)).to(eng.device).reshape(len(tslist), -1)
        if self._face_type == "dgrad_3d":
            verts = viewer.track_to_mesh(track, plan)[:n]
        else:
            verts = viewer._device_verts(plan.rows(track)[:n], self._face_type)
        rend = viewer.renderer(video_size)
        video.write_video(video_path, n, lambda i0, i1: rend.render(verts[i0:i1]), video_size[0], video_size[1], fps,
                          sound=g["sound"], sample_rate=_audio.SOUND_SR, encoder=jpeg_encoder)


class AnimationStream:
    """One live stream of SaberSpeechDrivenAnimation.animation_stream (a one-stream sdfa_amd.live.LiveSession with host copies)."""

    def __init__(self, owner, speaker, ensembling_ms, input_rate=None, gain=1.0):
        from sdfa_amd.live import LiveSession
        self._owner = owner
        sr = owner.hp.audio.sample_rate
        if input_rate is not None and not (isinstance(input_rate, (int, np.integer)) and input_rate > 0):
            raise ValueError(f"input_rate must be a positive integer, not {input_rate!r}")
        self._session = LiveSession(owner._model._engine, 1, sample_rate=sr, host_copy=True, max_ensembling_ms=max(ensembling_ms, 0),
                                    max_input_rate=sr if input_rate is None else int(input_rate))
        self._sid = self._session.open(speaker, ensembling_ms, input_rate=input_rate, gain=gain)
        self._shape = (owner._model._engine.out_dim // 9, 9) if owner._face_type == "dgrad_3d" else None

    def _result(self, res):
        width = self._owner._model._engine.out_dim
        ts, rows = res.get(self._sid, (np.empty(0, np.int32), torch.empty((0, width), dtype=torch.float32)))
        animes = rows.numpy()
        if self._shape is not None:
            animes = animes.reshape((animes.shape[0],) + self._shape)
        return [int(t) for t in ts], animes

    def push(self, chunk):
        """Samples (float32 in [-1, 1], at the stream's input rate) -> (tslist, animes) of the frames that became final."""
        if np.size(chunk) == 0:
            return self._result({})
        chunk = SaberSpeechDrivenAnimation._check_signal(chunk)
        self._session.push(self._sid, chunk)
        return self._result(self._session.step())

    def finish(self):
        """Ends the stream: (tslist, animes) of the remaining frames, the tail past the end of the audio included."""
        self._session.close(self._sid)
        return self._result(self._session.step())
