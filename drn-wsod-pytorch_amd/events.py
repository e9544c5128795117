"""EventStorage shim (detectron2/utils/events.py:232-431).  The reference calls
`get_event_storage().put_scalar(...)` from inside the hot path and floats the value at once — one
device->host sync per call.  Here scalars are kept as they come (device tensors
stay on the device) and are only materialised when somebody reads them."""
import bisect
import json
import statistics
from collections import defaultdict
from contextlib import contextmanager

_CURRENT_STORAGE_STACK = []


def get_event_storage():
    assert len(_CURRENT_STORAGE_STACK), "get_event_storage() has to be called inside a 'with EventStorage(...)' context!"
    return _CURRENT_STORAGE_STACK[-1]


def has_event_storage():
    return len(_CURRENT_STORAGE_STACK) > 0


class EventStorage:
    def __init__(self, start_iter=0):
        self._history = defaultdict(list)
        self._latest = {}
        self._iter = start_iter
        self._current_prefix = ""
        self._latest_iter = {}   # put_scalar_at: iteration of the value latest() shows
        self._no_smooth = set()  # names put with smoothing_hint=False (latest_with_smoothing_hint shows their last value)

    def put_scalar(self, name, value, smoothing_hint=True):
        name = self._current_prefix + name
        self._history[name].append((value, self._iter))
        self._latest[name] = value

    def put_scalars(self, *, smoothing_hint=True, **kwargs):
        for k, v in kwargs.items():
            self.put_scalar(k, v, smoothing_hint=smoothing_hint)

    def latest(self):
        return {k: float(v) for k, v in self._latest.items()}  # sync happens here, on demand

    def history(self, name):
        return [(float(v), it) for v, it in self._history[name]]

    def put_scalar_at(self, name, value, iteration, smoothing_hint=True):
        """put_scalar for a value that belongs to `iteration` rather than the current one - records drained from the device-side
        metrics ring arrive some iterations late.  The history stays ordered by iteration; latest() shows the value of the
        highest iteration put so far."""
        name = self._current_prefix + name
        iteration = int(iteration)
        h = self._history[name]
        pos = len(h)
        if h and h[-1][1] > iteration:
            pos = bisect.bisect_right([it for _, it in h], iteration)
        h.insert(pos, (value, iteration))
        if pos == len(h) - 1:
            self._latest[name] = value
            self._latest_iter[name] = iteration
        if not smoothing_hint:
            self._no_smooth.add(name)

    def latest_with_smoothing_hint(self, window_size=20):
        """detectron2/utils/events.py:359-370: latest(), with every scalar that carries a smoothing hint replaced by the median of
        its last `window_size` values (HistoryBuffer.median, np.median: the mean of the two middle values of an even count)"""
        out = {}
        for k, v in self._latest.items():
            if k in self._no_smooth:
                out[k] = float(v)
            else:
                out[k] = float(statistics.median(float(x) for x, _ in self._history[k][-window_size:]))
        return out

    def latest_iter(self):
        """highest iteration a scalar was put at with put_scalar_at (None: none was)"""
        return max(self._latest_iter.values()) if self._latest_iter else None

    def step(self):
        self._iter += 1

    @property
    def iter(self):
        return self._iter

    @iter.setter
    def iter(self, val):
        self._iter = int(val)

    def __enter__(self):
        _CURRENT_STORAGE_STACK.append(self)
        return self

    def __exit__(self, exc_type, exc_val, exc_tb):
        assert _CURRENT_STORAGE_STACK[-1] == self
        _CURRENT_STORAGE_STACK.pop()

    @contextmanager
    def name_scope(self, name):
        old = self._current_prefix
        self._current_prefix = name.rstrip("/") + "/"
        yield
        self._current_prefix = old


class JSONWriter:
    """detectron2/utils/events.py:32-106: one line per write(), `json.dumps({"iteration": it, **scalars}, sort_keys=True) + "\n"`
    with the scalars of latest_with_smoothing_hint(window_size).  iteration: the storage's current one, or - for scalars that came
    out of the metrics ring - pass the records' own (write(iteration=...))."""

    def __init__(self, path, window_size=20):
        self._fh = open(path, "a")
        self._window_size = window_size

    def write(self, storage=None, iteration=None):
        storage = storage if storage is not None else get_event_storage()
        to_save = {"iteration": storage.iter if iteration is None else int(iteration)}
        to_save.update(storage.latest_with_smoothing_hint(self._window_size))
        self._fh.write(json.dumps(to_save, sort_keys=True) + "\n")
        self._fh.flush()

    def close(self):
        self._fh.close()


class CommonMetricPrinter:
    """detectron2/utils/events.py:155-229 without the time, ETA and memory fields: ` iter: N  total_loss: 1.234  loss_cls: ...
    lr: 0.001000` - every scalar with "loss" in its name as the median of its last 20 values, lr as the last one (N/A
    without)."""

    def __init__(self, max_iter=None, sink=print):
        self._max_iter = max_iter  # (the reference needs it for the ETA; kept for signature parity)
        self._sink = sink

    def format(self, storage, iteration=None):
        iteration = storage.iter if iteration is None else int(iteration)
        losses = "  ".join("{}: {:.3f}".format(k, statistics.median(float(x) for x, _ in h[-20:]))
                           for k, h in storage._history.items() if "loss" in k and h)
        h = storage._history.get("lr")
        lr = "{:.6f}".format(float(h[-1][0])) if h else "N/A"
        return " iter: {iter}  {losses}  lr: {lr}".format(iter=iteration, losses=losses, lr=lr)

    def write(self, storage=None, iteration=None):
        storage = storage if storage is not None else get_event_storage()
        self._sink(self.format(storage, iteration))

    def close(self):
        pass


def write_all(writers, storage=None, iteration=None):
    """hooks.PeriodicWriter.after_step (detectron2/engine/hooks.py:164-173): every writer's write(), in order"""
    for w in writers:
        w.write(storage, iteration)
