"""Network description shared by the model builders and the device engine.

A network of the reference's family is: per-modality encoder streams (GaussianNoise -> stacked
Bidirectional(LSTM) [-> residual add]) -> concat -> optional fusion Bidirectional(LSTM) -> Dropout ->
Dense -> softmax -> CTC (reference multimodal_fusion/multimodal.py:88-213,
audio_network/speech_lstm_ctc_words.py:42-132, skeletal_network/skeletal_lstm_ctc.py:282-394).
"""
import copy
import json


class NetworkSpec:
    def __init__(self, streams, fusion, head, ctc=None, optimizer=None, name="model"):
        self.streams = copy.deepcopy(streams)
        self.fusion = copy.deepcopy(fusion)
        self.head = copy.deepcopy(head)
        self.ctc = dict({"skip": 2, "eps": 1e-8}, **(ctc or {}))
        self.optimizer = dict({"lr": 1e-4, "decay": 0.0, "clipvalue": 0.5, "beta_1": 0.9, "beta_2": 0.999,
                               "epsilon": 1e-7, "maxnorm": 3.0}, **(optimizer or {}))
        self.name = name
        for s in self.streams:
            if s.get("frontend"):
                fe = s["frontend"]
                if s.get("noise", 0.0) or any(lay.get("dropout", 0.0) for lay in fe["layers"]):
                    raise ValueError("stream %s: a CNN front-end takes no GaussianNoise and no Dropout before its convolutions"
                                     % s["name"])
                s["F"] = frontend_layers(fe)[-1]["F"]
            s.setdefault("noise", 0.0)
            s.setdefault("residual", len(s["layers"]) == 2)
            s.setdefault("trainable", True)
            for lay in s["layers"]:
                lay.setdefault("dropout", 0.0)
        if self.fusion:
            self.fusion.setdefault("dropout", 0.0)
        self.head.setdefault("dropout", 0.0)

    # ------------------------------------------------------------------------------------------
    def to_dict(self):
        return {"name": self.name, "streams": copy.deepcopy(self.streams), "fusion": copy.deepcopy(self.fusion),
                "head": copy.deepcopy(self.head), "ctc": dict(self.ctc), "optimizer": dict(self.optimizer)}

    @classmethod
    def from_dict(cls, d):
        return cls(d["streams"], d.get("fusion"), d["head"], d.get("ctc"), d.get("optimizer"), d.get("name", "model"))

    def to_json(self):
        return json.dumps({"class_name": "MgrNetwork", "config": self.to_dict()}, indent=1)

    @classmethod
    def from_json(cls, text):
        d = json.loads(text)
        return cls.from_dict(d["config"] if "config" in d else d)

    # ------------------------------------------------------------------------------------------
    def stream_width(self, s):
        return 2 * s["layers"][-1]["H"]

    @property
    def concat_width(self):
        return sum(self.stream_width(s) for s in self.streams)

    @property
    def head_width(self):
        return 2 * self.fusion["H"] if self.fusion else self.concat_width

    @property
    def num_classes(self):
        return self.head["C"]

    def lstm_layers(self):
        """Yield (prefix, F_in, H, dropout, trainable) for every Bidirectional layer in forward order."""
        for s in self.streams:
            fin = s["F"]
            for k, lay in enumerate(s["layers"]):
                yield ("%s/l%d" % (s["name"], k), fin, lay["H"], lay["dropout"], s["trainable"])
                fin = 2 * lay["H"]
        if self.fusion:
            yield ("fusion", self.concat_width, self.fusion["H"], self.fusion["dropout"], True)

    def kernel_maxnorm(self, prefix):
        """Max-norm (over axis 0, per column) of the input kernel of the Bidirectional layer `prefix` ("<stream>/l<k>" or
        "fusion"); 0.0 = unconstrained.  A layer's own "maxnorm" entry (set when the model came from a Keras JSON) wins over
        the optimizer-wide default, which is what the reference's builders use for every LSTM (maxnorm(3))."""
        lay = self.fusion if prefix == "fusion" else None
        if lay is None:
            sname, k = prefix.rsplit("/l", 1)
            lay = next(s for s in self.streams if s["name"] == sname)["layers"][int(k)]
        v = lay.get("maxnorm")
        return float(self.optimizer.get("maxnorm") or 0.0) if v is None else float(v)

    def weight_table(self):
        """Ordered (name, keras_shape, trainable, kind) - Keras weight-list order: a stream's CNN front-end (kernel (kh, kw, cin, cout),
        bias) first, then per Bidirectional layer fwd W,U,b then bwd W,U,b."""
        out = []
        for s in self.streams:
            for c in frontend_layers(s.get("frontend")):
                out.append(("%s/%s/W" % (s["name"], c["name"]), (c["ks"], c["ks"], c["Cin"], c["Cout"]), s["trainable"], "conv"))
                out.append(("%s/%s/b" % (s["name"], c["name"]), (c["Cout"],), s["trainable"], "conv_bias"))
        for prefix, fin, H, _, tr in self.lstm_layers():
            for d in ("fwd", "bwd"):
                out.append(("%s/%s/W" % (prefix, d), (fin, 4 * H), tr, "kernel"))
                out.append(("%s/%s/U" % (prefix, d), (H, 4 * H), tr, "recurrent"))
                out.append(("%s/%s/b" % (prefix, d), (4 * H,), tr, "bias"))
        out.append(("dense/W", (self.head_width, self.head["C"]), True, "dense"))
        out.append(("dense/b", (self.head["C"],), True, "dense_bias"))
        return out

    def count_params(self, trainable_only=False):
        n = 0
        for _, shape, tr, _ in self.weight_table():
            if trainable_only and not tr:
                continue
            k = 1
            for s in shape:
                k *= s
            n += k
        return n

    def flops_per_frame(self, executed=False):
        """Algorithmic FLOP per padded frame of one training step (2 x MAC), SURVEY 8(d) accounting:
        forward of every layer, backward (dZ.U^T, dW, dU [, dX]) of trainable ones, Dense fwd+bwd.
        executed=True: what the device really multiplies in a training step - the dropout-aware projection and dW kernels
        (used from p >= 0.3 on, 16 <= F <= 2048) skip the products with dropped features, i.e. run the (1 - p) share of
        their K loops; the skipped terms are exact zeros, the result is the dense one."""
        mac = 0
        fe_streams = set()
        for s in self.streams:
            for i, c in enumerate(frontend_layers(s.get("frontend"))):
                conv = 4 * c["Hp"] * c["Wp"] if executed else c["Ho"] * c["Wo"]   # (the device forms the pooled windows only)
                conv *= c["ks"] * c["ks"] * c["Cin"] * c["Cout"]
                mac += conv * (1 + (2 if s["trainable"] and i > 0 else 1 if s["trainable"] else 0))   # fwd, dW [, dX]
                fe_streams.add(s["name"])
        for prefix, fin, H, p, tr in self.lstm_layers():
            keep = (1.0 - p) if (executed and p >= 0.3 and 16 <= fin <= 2048) else 1.0
            proj = fin * 4 * H
            fwd = 2 * (proj * keep + H * 4 * H)
            mac += fwd
            if tr:
                bwd = 2 * (proj * keep + 2 * H * 4 * H)  # dW + (dh_rec, dU)
                first = prefix.endswith("/l0")
                if first and prefix.rsplit("/l", 1)[0] in fe_streams:
                    bwd += 2 * fin * 4 * H  # dX to the CNN front-end
                if not first and prefix != "fusion":
                    bwd += 2 * fin * 4 * H  # dX to a trainable layer below
                elif prefix == "fusion" and any(s["trainable"] for s in self.streams):
                    bwd += 2 * fin * 4 * H
                mac += bwd
        mac += self.head_width * self.head["C"] * 3
        return 2 * mac if executed else int(2 * mac)


def frontend_layers(frontend):
    """Shapes of a stream's TimeDistributed CNN front-end (rgb_network/cnn_lstm.py): per layer a valid Conv2D (bias, ReLU) and a 2x2 /
    stride 2 floor max-pool, channels-last.  frontend = {"input_shape": [h, w, c], "layers": [{"name", "filters", "kernel_size"}]};
    returns per layer dict(name, Hin, Win, Cin, ks, Cout, Ho, Wo, Hp, Wp, F) with F = Hp * Wp * Cout, the flattened width of its
    pooled output (channels-last flatten, f = (i * Wp + j) * Cout + c)."""
    if not frontend:
        return []
    h, w, c = (int(v) for v in frontend["input_shape"])
    out = []
    for lay in frontend["layers"]:
        ks, co = int(lay["kernel_size"]), int(lay["filters"])
        ho, wo = h - ks + 1, w - ks + 1
        hp, wp = ho // 2, wo // 2
        if hp < 1 or wp < 1:
            raise ValueError("front-end layer %s: input %dx%d too small for a %dx%d kernel and a 2x2 pool" % (lay["name"], h, w, ks, ks))
        out.append(dict(name=lay["name"], Hin=h, Win=w, Cin=c, ks=ks, Cout=co, Ho=ho, Wo=wo, Hp=hp, Wp=wp, F=hp * wp * co))
        h, w, c = hp, wp, co
    return out


def input_width(s):
    """Per-frame width of a stream's raw input: F, or h * w * c of its front-end's frames."""
    fe = s.get("frontend")
    if not fe:
        return s["F"]
    h, w, c = (int(v) for v in fe["input_shape"])
    return h * w * c
