"""RGB network builder, data generator and training entry point (reference rgb_network/cnn_lstm.py:22-375):
per frame Conv2D(16, 5x5) -> MaxPool 2 -> Conv2D(32, 5x5) -> MaxPool 2 -> Conv2D(48, 4x4) -> MaxPool 2 -> Flatten (TimeDistributed),
then BiLSTM(512) -> BiLSTM(512) -> add -> Dense(22) -> softmax -> CTC.  Every Dropout of the reference has rate 0."""
import argparse
import csv
import os
import random
import time

import numpy as np

from .. import keras_like as K
from ..configs import rgb_spec
from ..keras_like import Adam, Model, ModelCheckpoint
from ..multimodal_fusion.losses import ctc_lambda_func  # noqa: F401  (the reference's Lambda: K.ctc_batch_cost on y_pred[:, 2:])

img_dim = 60
maxlen = 1900
nb_classes = 22


class DataGenerator(K.Callback):
    """Batches of (B, maxlen, img_dim, img_dim, 1) frame sequences with the reference's quirks: files are ``.npy`` arrays of shape
    (frames, img_dim, img_dim, 1), post-padded / truncated to maxlen with zeros; the file number is ``int(name[6:11])``; labels come
    from a CSV with columns Id and Sequence; a file without a label row keeps the all-ones frames of the batch buffer and gets the
    blank label (nb_classes - 1) with label_length 1; the batch is then normalised with ``X -= 128; X /= 255``; input_length is
    maxlen - 2; the train / validation split shuffles the sorted directory listing after ``random.seed(10)`` and both lists are
    cut to a multiple of the batch size; on_epoch_end shuffles both again.
    synthetic_files=n: n generated files (Sample00000 ...; every fifth has no label row) instead of a directory.
    store=roi_extraction.RoiStore: the file list and the frames come from the store (the crops of a colour-video directory, made on
    the GPU on first use) instead of data_path; the labels still come from lab_file."""

    def __init__(self, minibatch_size, img_dim, maxlen, val_split, nb_classes=22, data_path=None, lab_file=None,
                 absolute_max_sequence_len=28, synthetic_files=None, seed=20131903, store=None):
        super().__init__()
        self.minibatch_size = minibatch_size
        self.maxlen = maxlen
        self.img_dim = img_dim
        self.val_split = val_split
        self.absolute_max_sequence_len = absolute_max_sequence_len
        self.train_index = 0
        self.val_index = 0
        self.nb_classes = nb_classes
        self.data_path = data_path
        self.lab_file = lab_file
        self.blank_label = np.array([self.nb_classes - 1])
        self.synthetic_files = synthetic_files
        self.seed = seed
        self.store = store
        if store is not None and synthetic_files is not None:
            raise ValueError("store and synthetic_files are exclusive")
        self.load_dataset()

    # ---- data sources ------------------------------------------------------------------------
    def _synthetic_name(self, i):
        return "Sample%05d.npy" % i

    def load_dataset(self):
        if self.synthetic_files is not None:
            file_list = [self._synthetic_name(i) for i in range(int(self.synthetic_files))]
            self.labs = {}
            for i in range(int(self.synthetic_files)):
                if i % 5 != 4:
                    rng = np.random.RandomState(self.seed + 7 * i)
                    n = rng.randint(1, min(8, self.absolute_max_sequence_len) + 1)
                    self.labs[i] = " ".join(str(v) for v in rng.randint(0, self.nb_classes - 1, n))
        else:
            self.labs = {}
            with open(self.lab_file) as f:
                for row in csv.DictReader(f):
                    self.labs.setdefault(int(row["Id"]), row["Sequence"])
            file_list = self.store.names() if self.store is not None else sorted(os.listdir(self.data_path))
        random.seed(10)
        random.shuffle(file_list)
        split_point = int(len(file_list) * (1 - self.val_split))
        self.train_list, self.val_list = file_list[:split_point], file_list[split_point:]
        for attr in ("train_list", "val_list"):
            lst = getattr(self, attr)
            mod = len(lst) % self.minibatch_size
            if mod:
                del lst[-mod:]
        self.train_size = len(self.train_list)
        self.val_size = len(self.val_list)

    def frames(self, file):
        """(frames, img_dim, img_dim, 1) of one file, values in 0..255."""
        if self.synthetic_files is not None:
            num = int(file[6:11])
            rng = np.random.RandomState(self.seed + 7 * num + 1)
            n = rng.randint(self.maxlen // 2, self.maxlen + self.maxlen // 4 + 1)
            return rng.randint(0, 256, (n, self.img_dim, self.img_dim, 1)).astype(np.float64)
        if self.store is not None:
            return self.store.frames(file).astype(float)
        return np.load(os.path.join(self.data_path, file)).astype(float)

    def get_size(self, train):
        return self.train_size if train else self.val_size

    # ---- batches -----------------------------------------------------------------------------
    def batch_of(self, batch):
        size = len(batch)
        L = self.absolute_max_sequence_len
        X_data = np.ones([size, self.maxlen, self.img_dim, self.img_dim, 1], dtype=np.float32)
        labels = np.ones([size, L])
        input_length = np.zeros([size, 1])
        label_length = np.zeros([size, 1])
        for i, file in enumerate(batch):
            file_num = int(file[6:11])
            seq = self.frames(file)
            lab = self.labs.get(file_num)
            row = -np.ones(L)
            if lab is None:
                row[0] = self.blank_label[0]
                label_length[i] = 1
            else:
                n = min(self.maxlen, seq.shape[0])          # pad_sequences(padding='post', truncating='post')
                X_data[i, :n] = seq[:n]
                X_data[i, n:] = 0.0
                lab_seq = np.array([int(v) for v in lab.split()], np.float32)
                label_length[i] = lab_seq.shape[0]
                kept = lab_seq[-L:]                          # (pad_sequences truncates 'pre')
                row[:kept.shape[0]] = kept
            labels[i, :] = row
            input_length[i] = self.maxlen - 2
        X_data -= 128.
        X_data /= 255.
        inputs = {'the_input': X_data, 'the_labels': labels, 'input_length': input_length, 'label_length': label_length}
        return inputs, {'ctc': np.zeros([size])}

    def get_batch(self, train):
        file_list, index = (self.train_list, self.train_index) if train else (self.val_list, self.val_index)
        return self.batch_of(file_list[index:index + self.minibatch_size])

    def next_train(self):
        while 1:
            ret = self.get_batch(train=True)
            self.train_index += self.minibatch_size
            if self.train_index >= self.train_size:
                self.train_index = 0
            yield ret

    def next_val(self):
        while 1:
            ret = self.get_batch(train=False)
            self.val_index += self.minibatch_size
            if self.val_index >= self.val_size:
                self.val_index = 0
            yield ret

    def predict_batches(self, files):
        """Input batches of `files` in order (decode_rgb): the frames only."""
        for k in range(0, len(files), self.minibatch_size):
            yield self.batch_of(files[k:k + self.minibatch_size])[0]['the_input']

    def on_epoch_end(self, epoch, logs=None):
        self.train_index = 0
        self.val_index = 0
        random.shuffle(self.train_list)
        random.shuffle(self.val_list)


def build_net(img_dim=img_dim, maxlen=maxlen, nb_classes=nb_classes, h=512, device=0, seed=1234):
    """The reference's graph (cnn_lstm.py:251-375) as a NetworkSpec, compiled with Adam(lr=1e-4, clipvalue=0.5)."""
    K.set_learning_phase(1)
    model = Model(rgb_spec(img_dim, nb_classes, h), device=device, seed=seed)
    model.compile(loss={'ctc': lambda y_true, y_pred: y_pred}, optimizer=Adam(lr=0.0001, clipvalue=0.5))
    return model


def load_model(json_path="rgb_ctc_lstm_model.json", weights_path="rgb_ctc_lstm_weights_best.h5", device=0):
    with open(json_path) as f:
        model = K.model_from_json(f.read(), device=device)
    model.load_weights(weights_path)
    model.compile(loss={'ctc': lambda y_true, y_pred: y_pred}, optimizer=Adam(lr=0.0001, clipvalue=0.5))
    return model


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--minibatch-size", type=int, default=2)
    ap.add_argument("--maxlen", type=int, default=maxlen)
    ap.add_argument("--img-dim", type=int, default=img_dim)
    ap.add_argument("--epochs", type=int, default=500)
    ap.add_argument("--data-path", default="../data/train_rgb")
    ap.add_argument("--lab-file", default="../data/training.csv")
    ap.add_argument("--synthetic-files", type=int, default=None)
    a = ap.parse_args(argv)
    gen = DataGenerator(a.minibatch_size, a.img_dim, a.maxlen, 0.2, nb_classes, a.data_path, a.lab_file,
                        synthetic_files=a.synthetic_files)
    model = build_net(a.img_dim, a.maxlen, nb_classes)
    model.summary()
    with open("rgb_ctc_lstm_model.json", "w") as f:
        f.write(model.to_json())
    checkpoint = ModelCheckpoint("rgb_ctc_lstm_weights_best.h5", monitor='val_loss', verbose=1, save_best_only=True,
                                 save_weights_only=True, mode='auto')
    start = time.time()
    model.fit_generator(generator=gen.next_train(), steps_per_epoch=gen.get_size(True) // a.minibatch_size, epochs=a.epochs,
                        validation_data=gen.next_val(), validation_steps=gen.get_size(False) // a.minibatch_size,
                        callbacks=[checkpoint, gen])
    print("--- Training time: %s seconds ---" % (time.time() - start))
    return model


if __name__ == '__main__':
    main()
