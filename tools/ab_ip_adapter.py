"""Developer A/B of whole denoise steps with the IP-Adapter pass (ip_adapter.py) on ONE box, in ONE process, interleaved so that
drift cancels: SDXL-base, bf16, batch 1, latent 128, captured single steps (mode="step"), in the manner of tools/ab_step.py.
Four loops over the same weights: compiled without the pass; compiled with ip_adapter=4 but off (every scale 0); on at N = 4; on at
N = 16 (scale 0.6 at every site).
usage: python tools/ab_ip_adapter.py [--rounds R] [--steps K] [--latent L]"""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--latent", type=int, default=128)
    a = ap.parse_args()
    import torch
    from stabletriton_amd import synth
    from stabletriton_amd.optimization import optimize_model
    from stabletriton_amd.pipeline import DenoiseLoop
    from stabletriton_amd.scheduler import euler_discrete_tables
    from stabletriton_amd.unet import SDXL_BASE, UNet2DConditionModel
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    with torch.device("meta"):
        m = UNet2DConditionModel(SDXL_BASE)
    m = m.to_empty(device=dev).to(dtype).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    x = synth.denoise_inputs(1, a.latent, 1234, device=dev)

    def loop_for(ip, on):
        gm = optimize_model(m, cuda_graph=False, ip_adapter=ip)
        loop = DenoiseLoop(gm, 1, a.latent, dtype, dev, euler_discrete_tables(50), mode="step")
        loop.set_conditioning(x["encoder_hidden_states"].to(dtype), x["text_embeds"].to(dtype), x["time_ids"].to(dtype))
        if on:
            st = gm.ip_adapter
            sd = {}
            for path, (c, cross) in zip(st.sites, st.dims):
                sd[f"{path}.to_k_ip.weight"] = synth.normal(f"ab.k.{path}", (c, cross), 5) * cross ** -0.5
                sd[f"{path}.to_v_ip.weight"] = synth.normal(f"ab.v.{path}", (c, cross), 6) * cross ** -0.5
            loop.load_ip_adapter(sd)
            loop.set_ip_adapter_image(synth.normal("ab.tokens", (1, ip, SDXL_BASE.cross_dim), 7))
            loop.set_ip_adapter_scale(0.6)
        loop.set_noise(x["latent"])
        with torch.no_grad():
            loop.capture()
            loop.run_steps(10)
        torch.cuda.synchronize()
        return loop

    loops = {"without the pass": loop_for(None, False), "ip_adapter=4, off": loop_for(4, False), "ip_adapter=4, on": loop_for(4, True),
             "ip_adapter=16, on": loop_for(16, True)}
    res = {k: [] for k in loops}
    with torch.no_grad():
        for r in range(a.rounds):
            for name, loop in loops.items():
                t0 = time.perf_counter()
                loop.run_steps(a.steps)
                torch.cuda.synchronize()
                res[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    base = min(res["without the pass"])
    for name, xs in res.items():
        print(f"RESULT {name:20s} min {min(xs):.4f}  median {statistics.median(xs):.4f} ms/step  (+{min(xs) - base:.4f} ms against the loop "
              f"without the pass; {a.rounds} interleaved rounds of {a.steps} captured steps)", flush=True)


if __name__ == "__main__":
    main()
