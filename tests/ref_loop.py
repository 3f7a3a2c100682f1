"""The outer loop of the float64 yardsticks (is_ref, masked_ref, weighted_ref, beta_ref, ard_ref, transform_ref): the loop
of oracle.nmf_ref.mur on steps and an objective handed in."""
from oracle import nmf_ref as R


def ref_loop(w, h, w_step, h_step, objective, min_iter, max_iter, tol1, tol2):
    """history[0] = objective(w, h) of the start; iteration i: w = w_step(w, h) (None: W stays, fold-in), h = h_step(w, h)
    with the new w, the objective appended, and after min_iter the reference's stop rule on the last two entries."""
    hist = [objective(w, h)]
    trace = {"snap": {}, "stop_rule": 0}
    i = -1
    for i in range(max_iter):
        if w_step is not None:
            w = w_step(w, h)
        h = h_step(w, h)
        hist.append(objective(w, h))
        if i > min_iter:
            rule = R.stop_rule(hist[-1], hist[-2], tol1, tol2)
            if rule:
                trace["stop_rule"] = rule
                break
    return R.Outcome(w, h, i, hist, trace)
