"""Mirrors of the reference's GPT_SoVITS/tools helpers that sit on the inference path (tools/audio_sr.py)."""
