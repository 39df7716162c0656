// ray_valid.inc -- hostile rays, decided on the device (device-resident rays never pass the host): which rays the cast
// (ray_query.hip), the occlusion kernel (occlusion.hip) and the ID pass (selection.hip: tmax = +inf and unit directions, both
// constants, which fold the statements to its shorter form) walk at all. Text, not a function: as a __forceinline__ function
// of (org, dir by reference, tmax, flags) the same statements compiled to other instruction streams in all nine kernels
// (DESIGN.md 29).
// In scope: org (f3), dir (f3, not const: normalised here unless the flag says it is a unit vector), tmax (float), flags
// (uint32_t, SRT_RAYS_*). Declares valid (bool).
	bool valid = finite3(org) && finite3(dir) && tmax == tmax;
	if (!(flags & SRT_RAYS_UNIT_DIRECTIONS)) {
		// detmath's division-free rsqrt keeps normalize(0) = 0, gives a large finite value where the squared length underflows and
		// no number where it overflows: what comes out is a direction only if it has unit length (NaN compares false)
		dir = normalize3(dir);
		const float len2 = dot3(dir, dir);
		valid = valid && len2 > 0.25f && len2 < 4.0f;
	}
	valid = valid && finite3(dir) && !(dir.x == 0.0f && dir.y == 0.0f && dir.z == 0.0f);
