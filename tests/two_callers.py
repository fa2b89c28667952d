"""Two Python threads in one device entry at once, for the GPU tests of the batched entries.  The bindings release the interpreter lock
for the length of a call, so the two calls meet in the library: at the lock of the entry's buffers."""
import threading


def run(call, batches_a, batches_b, timeout=60.0):
    """call(batch) for every batch of batches_a on one thread and of batches_b on another, both started together -> (results_a, results_b).
    Fails, without waiting longer than `timeout` seconds, if a thread does not come back: a deadlock must not hang the suite."""
    start = threading.Barrier(2)
    results, errors = {}, {}

    def work(name, batches):
        try:
            start.wait(timeout)
            results[name] = [call(b) for b in batches]
        except BaseException as e:                                                   # reported by the caller's thread
            errors[name] = e

    threads = [threading.Thread(target=work, args=(n, b), daemon=True) for n, b in (("a", batches_a), ("b", batches_b))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout)
    assert not any(t.is_alive() for t in threads), "a caller did not come back within %g s" % timeout
    for name in ("a", "b"):
        if name in errors:
            raise errors[name]
    return results["a"], results["b"]
