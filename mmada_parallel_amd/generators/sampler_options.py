"""The device samplers' options, for all five generators: the refusals of `image_sampler` / `text_sampler`, the seed as the kernels
take it, and where the image draws' counter starts."""
from __future__ import annotations

# The image draws' counter starts here per call and advances by 1 per image step; the text draws' starts at 0.  Far apart, so a text
# row and an image row of one step never share (seed, counter, row).
IMAGE_COUNTER0 = 1 << 62


def seed_u64(sampler_seed) -> int:
    """`sampler_seed` as the uint64 the kernels key their counter-based generator with."""
    return int(sampler_seed) & 0xFFFFFFFFFFFFFFFF


def check_samplers(model, image_sampler="torch", text_sampler="torch", sampler_seed=None, *, temperature=None,
                   text_temperature=0.0, text_temperature_name="text_temperature",
                   text_rank_note="tensor parallelism is out of scope"):
    """Refuse what a device sampler cannot do; returns (dev_img, dev_text).  First a value that is neither "torch" nor "device",
    then per sampler that is "device" — text first — a temperature that draws nothing, a tensor-parallel model other than a group of two or
    more ranks on the library's pull or copy transport (the "one rank" refusals), a missing `sampler_seed`.
    temperature: the image temperature, for the generators whose image step is an arg-max at 0 (None: not checked).
    text_temperature_name: what the caller's signature calls the text temperature (mmu_generate: `temperature`)."""
    for name, value in (("text_sampler", text_sampler), ("image_sampler", image_sampler)):
        if value not in ("torch", "device"):
            raise ValueError(f"{name}={value!r}: 'torch' or 'device'")
    dev_img, dev_text = image_sampler == "device", text_sampler == "device"
    # two or more ranks whose exchange runs in the library over a mapped transport: the sampling head is vocabulary-parallel
    # (model.vocab_parallel_row_heads) and the image-side kernels read logits every rank holds alike
    vocab_parallel = model.tp_size >= 2 and model._comm_in_library and model.tp_collective in ("pull", "copy")
    needs = []
    if dev_text:
        needs.append(("text_sampler", text_temperature > 0,
                      f"{text_temperature_name} > 0 (at 0 the text step is an arg-max: nothing is drawn)", text_rank_note))
    if dev_img:
        needs.append(("image_sampler", temperature is None or temperature > 0,
                      "temperature > 0 (at 0 the image step is an arg-max: nothing is drawn)", "tensor parallelism is out of scope"))
    for name, draws, why_draws, rank_note in needs:
        why = None
        if not draws:
            why = why_draws
        elif (model.tp_size != 1 or model._comm_in_library) and not vocab_parallel:
            why = f"one rank ({rank_note})"
        elif sampler_seed is None:
            why = "sampler_seed"
        if why:
            raise ValueError(f"{name}='device' needs {why}")
    return dev_img, dev_text
