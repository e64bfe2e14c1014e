"""What the GPU tests of the two vector agents share (tests/test_il_vector_agent_gpu.py, tests/test_vector_agent_vida_gpu.py): the gate on action probabilities, the
record of one episode, and the staggered schedule of three slots.  The reference of every comparison stays with the tests: the two models' forwards differ."""
import numpy as np


def gate(got, ref, name):
    err, tol = np.abs(got - ref).max(), 2e-2 * max(ref.max(), 1e-3)
    print(f"{name}: max |dp| {err:.3e}, gate {tol:.3e}")
    assert err < tol, (name, err, tol)


class Episode:
    def __init__(self, goal):
        self.goal, self.frames, self.acts, self.probs = goal, [], [], []

    def record(self, agent, frame, out):
        a, p = out
        assert p.shape == (20,) and abs(float(p.sum()) - 1.0) < 1e-4
        self.frames.append(frame); self.acts.append(agent.get_action_list().index(a)); self.probs.append(p.float().cpu().numpy())


def staggered_episodes(agent, goal_of, frame):
    """Three slots that start at calls 0, 2 and 4 with ``goal_of(slot)``; slot 1 sits out calls 5 and 6; slot 0 is reset after 5 steps with ``goal_of("reset")``; 12 calls
    on ``frame()`` observations.  -> the four episodes, finished or not, in the order [slot 0's first, slot 0's second, slot 1's, slot 2's]: 5, 7, 8 and 8 steps."""
    assert agent.num_episodes == 3 and len(agent.get_action_list()) == 20
    start = {0: 0, 1: 2, 2: 4}
    live, done = {}, []
    for call in range(12):
        for s, c0 in start.items():
            if call == c0:
                live[s] = Episode(goal_of(s))
                agent.reset(s, live[s].goal)
        if call == 5:                                                       # slot 0 has taken 5 steps: a new episode with a goal of another length
            assert agent.age(0) == 5
            done.append(live[0])
            live[0] = Episode(goal_of("reset"))
            agent.reset(0, live[0].goal)
        active = [s for s in sorted(live) if not (s == 1 and call in (5, 6))]
        frames = {s: frame() for s in active}
        out = agent.get_actions(frames)
        assert sorted(out) == active
        for s in active:
            live[s].record(agent, frames[s], out[s])
    assert [agent.age(s) for s in range(3)] == [7, 8, 8]                    # slot 1 did not age while it sat out
    done += [live[s] for s in sorted(live)]
    assert [len(e.acts) for e in done] == [5, 7, 8, 8]
    return done
