"""-m "not gpu": a Keras 2.1.4 functional-Model JSON of the reference's RGB graph (rgb_network/cnn_lstm.py:251-375, written out by
hand in the layout Keras' model.to_json() uses) loads into rgb_spec(); forms the device kernels do not implement are refused."""
import copy
import json

import pytest

import mgr_amd  # noqa: F401
from mgr_amd import configs
from mgr_amd.keras_io import spec_from_keras_json
from mgr_amd.keras_like import model_from_json


def _layer(name, cls, config, inbound):
    return {"name": name, "class_name": cls, "config": dict(config, name=name),
            "inbound_nodes": [[[i, 0, 0, {}] for i in inbound]] if inbound else []}


def _td(name, cls, config, inbound):
    return _layer(name, "TimeDistributed", {"trainable": True, "layer": {"class_name": cls, "config": dict(config, name=name + "_inner")}},
                  inbound)


def _conv(filters, ks):
    return {"filters": filters, "kernel_size": [ks, ks], "strides": [1, 1], "padding": "valid", "data_format": "channels_last",
            "dilation_rate": [1, 1], "activation": "relu", "use_bias": True, "kernel_initializer": {"class_name": "RandomUniform"},
            "kernel_regularizer": None, "bias_regularizer": None, "activity_regularizer": None, "kernel_constraint": None,
            "bias_constraint": None}


POOL = {"pool_size": [2, 2], "padding": "valid", "strides": [2, 2], "data_format": "channels_last"}


def _blstm(wrapper, inner):
    return {"trainable": True, "merge_mode": "concat", "layer": {"class_name": "LSTM", "config": {
        "name": inner, "units": 512, "activation": "tanh", "recurrent_activation": "hard_sigmoid", "dropout": 0.0,
        "recurrent_dropout": 0.0, "return_sequences": True, "trainable": True,
        "kernel_constraint": {"class_name": "MaxNorm", "config": {"max_value": 3, "axis": 0}},
        "recurrent_constraint": None, "bias_constraint": None}}}


def reference_graph(img_dim=60, maxlen=1900):
    L = [_layer("the_input", "InputLayer", {"batch_input_shape": [None, maxlen, img_dim, img_dim, 1], "dtype": "float32"}, []),
         _td("drop_1", "Dropout", {"rate": 0.0}, ["the_input"]),
         _td("conv_1", "Conv2D", _conv(16, 5), ["drop_1"]),
         _td("max_pool_1", "MaxPooling2D", POOL, ["conv_1"]),
         _td("drop_2", "Dropout", {"rate": 0.0}, ["max_pool_1"]),
         _td("conv_3", "Conv2D", _conv(32, 5), ["drop_2"]),
         _td("max_pool_2", "MaxPooling2D", POOL, ["conv_3"]),
         _td("drop_3", "Dropout", {"rate": 0.0}, ["max_pool_2"]),
         _td("conv_5", "Conv2D", _conv(48, 4), ["drop_3"]),
         _td("max_pool_3", "MaxPooling2D", POOL, ["conv_5"]),
         _td("flatten", "Flatten", {}, ["max_pool_3"]),
         _layer("bidirectional_1", "Bidirectional", _blstm("bidirectional_1", "blstm_1"), ["flatten"]),
         _layer("bidirectional_2", "Bidirectional", _blstm("bidirectional_2", "blstm_2"), ["bidirectional_1"]),
         _layer("residual_1", "Add", {}, ["bidirectional_1", "bidirectional_2"]),
         _layer("drop_4", "Dropout", {"rate": 0.0}, ["residual_1"]),
         _layer("dense_1", "Dense", {"units": 22, "activation": "linear"}, ["drop_4"]),
         _layer("softmax", "Activation", {"activation": "softmax"}, ["dense_1"]),
         _layer("the_labels", "InputLayer", {"batch_input_shape": [None, 28]}, []),
         _layer("input_length", "InputLayer", {"batch_input_shape": [None, 1]}, []),
         _layer("label_length", "InputLayer", {"batch_input_shape": [None, 1]}, []),
         _layer("ctc", "Lambda", {}, ["softmax", "the_labels", "input_length", "label_length"])]
    return {"class_name": "Model", "keras_version": "2.1.4", "backend": "tensorflow",
            "config": {"name": "model_1", "layers": L, "input_layers": [["the_input", 0, 0]], "output_layers": [["ctc", 0, 0]]}}


def _strip(streams):
    out = copy.deepcopy(streams)
    for s in out:
        for lay in s["layers"]:
            lay.pop("maxnorm", None)
    return out


@pytest.mark.parametrize("img_dim", [60, 48])
def test_reference_rgb_json_loads_to_rgb_spec(img_dim):
    spec, maxlen, Lmax = spec_from_keras_json(json.dumps(reference_graph(img_dim)))
    want = configs.rgb_spec(img_dim=img_dim)
    assert _strip(spec.streams) == _strip(want.streams)
    assert spec.head == want.head and spec.fusion is None
    assert spec.weight_table() == want.weight_table()
    assert spec.count_params() == (11602950 if img_dim == 60 else want.count_params())
    assert (maxlen, Lmax) == (1900, 28)
    assert [l["maxnorm"] for l in spec.streams[0]["layers"]] == [3.0, 3.0]
    m = model_from_json(json.dumps(reference_graph(img_dim)), device=0)
    assert m.spec.weight_table() == want.weight_table()


@pytest.mark.parametrize("layer,key,value", [
    ("conv_3", "activation", "tanh"), ("conv_3", "padding", "same"), ("conv_5", "strides", [2, 2]),
    ("max_pool_2", "pool_size", [3, 3]), ("drop_2", "rate", 0.25)])
def test_unsupported_front_end_forms_are_refused(layer, key, value):
    g = reference_graph()
    for l in g["config"]["layers"]:
        if l["name"] == layer:
            l["config"]["layer"]["config"][key] = value
    with pytest.raises(ValueError):
        spec_from_keras_json(json.dumps(g))
