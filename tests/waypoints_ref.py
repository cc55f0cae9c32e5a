"""numpy restatement of the reference's waypoint lap bookkeeping (evaluate.py:487-497 the start, :535-595 the
loop body after env.step), fed recorded step outputs instead of an env. TEST INFRASTRUCTURE ONLY."""
import numpy as np


def lap(waypoints, reach_radius, pos, reward, term, trunc):
    """The loop over the rows (pos [n,3] float32 = info["state"][:3], reward float32, terminated, truncated)
    until done. Returns (steps taken, track [n,6] float64 = wp_idx, waypoints_reached, laps_completed,
    step_count, status, total_reward after each row -- rows past the end repeat the last --, target [n+1,3]
    float32 = target_state.state[0:3] after the start and after each row, start position [3] float32).
    status: 0 running, 1 lap completed, 2 terminated, 3 truncated."""
    waypoints = np.asarray(waypoints, np.float64).reshape(-1, 3)
    reach_radius = float(np.float32(reach_radius))  # the C interface carries --reach-radius as a float
    num_waypoints = len(waypoints)
    start_pos = waypoints[0]
    qpos_init = np.array([start_pos[0], start_pos[1], start_pos[2], 1.0, 0.0, 0.0, 0.0])
    wp_idx = 1 % num_waypoints
    target = waypoints[wp_idx].astype(np.float32)
    step_count = 0
    total_reward = 0.0
    waypoints_reached = 0
    laps_completed = 0
    status = 0
    n = len(pos)
    track = np.zeros((n, 6), np.float64)
    targets = np.zeros((n + 1, 3), np.float32)
    targets[0] = target
    taken = 0
    for i in range(n):
        if status == 0:
            done = False
            total_reward += float(reward[i])  # env.step returns a Python float: a float64 sum
            step_count += 1
            drone_pos = np.asarray(pos[i], np.float32)
            current_target = waypoints[wp_idx]
            dist_to_wp = float(np.sqrt(np.sum((drone_pos - current_target) ** 2)))
            if dist_to_wp < reach_radius:
                waypoints_reached += 1
                wp_idx = (wp_idx + 1) % num_waypoints
                if wp_idx == 0:
                    laps_completed += 1
                    done = True
                    status = 1
                if not done:
                    target = waypoints[wp_idx].astype(np.float32)
            if status == 0 and term[i]:
                status = 2
            elif status == 0 and trunc[i]:
                status = 3
            taken += 1
        track[i] = (wp_idx, waypoints_reached, laps_completed, step_count, status, total_reward)
        targets[i + 1] = target
    return taken, track, targets, qpos_init[:3].astype(np.float32)
